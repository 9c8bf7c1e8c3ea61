// Radially averaged power spectra of forecast / observation pairs: a batched 2-D FFT with a fused radial reduction, read in place.
//
// One pair is the pred frame p and the target frame t of one (member, n, t, c), H x W fp32 pixels.  They travel as ONE complex frame
// z = p + i t (after the optional periodic Hann window): with Z its transform, P(k) = (Z(k) + conj Z(-k)) / 2 and
// T(k) = (Z(k) - conj Z(-k)) / (2 i), so one complex FFT per pair gives all three sums
//   S_p[b] += s |P|^2      S_t[b] += s |T|^2      S_x[b] += s Re(P conj T)        s = 1 / (H W), over the cells of radial bin b.
// The bins are the host's: cell_order (cells ky W + kx sorted by bin, corners dropped) and bin_start[nb + 1], built with the integer rule
// of prediff_amd/spectrum.py, so CPU restatement and kernel agree cell for cell.
//
// 1-D core (fft_lines): Stockham autosort in LDS, radix-4 stages, one radix-2 stage when log2 is odd, one radix-3 stage last (so the
// sub-transform length Ns of every earlier stage is a power of two).  Side lengths 2^a or 3 2^a, 8 .. 512.  A stage is
// read - barrier - write over the SAME buffer: a workgroup holds at most 16 elements per thread (16384 with 1024 threads), every
// butterfly's inputs are in registers (compile-time indexed: no scratch) before any output is written, so the autosort needs no second
// frame -- which is what lets a 128 x 128 complex frame (128 KiB) live in the 160 KiB of a gfx950 workgroup.  Twiddles: a per-workgroup
// LDS table exp(-2 pi i m / N) built with sincospif on an argument reduced to a quarter turn (the quadrant is applied exactly); no
// __sinf / __cosf.
//
// LDS-resident form (H W <= 16384): one workgroup per pair loads both frames through their strides, runs row FFTs, column FFTs and the
// radial reduce without leaving LDS.  Bank layout: the row pitch is PADDED by one complex (W + 1), no transpose.  The column pass maps
// adjacent lanes to adjacent columns, so where W >= 64 a wave reads and writes consecutive addresses whatever the pitch; where W < 64 a
// wave spans several butterfly positions, a power-of-two number of rows apart in the Stockham writes, and the odd pitch keeps those off
// one bank.  A transpose would cost a second frame or a pass through registers; the pad costs 1 KiB at 128 x 128 (129 complex per row,
// 132 KiB + the 1 KiB table).  What the pad does not cure: the first stages of the ROW pass write with stride 4 / 16 inside a row (up to
// 4 x the conflict-free time of those writes); accepted, the scorer is off the sampling path (profiles/time_spectrum.log).
//
// Strip form (larger frames, up to 512 x 512): three launches over a device workspace of complex fp32, 8 H W bytes per pair:
// row FFTs (16384 / W rows per workgroup, 15360 / W where W = 3 2^a: the radix-3 stage holds 15 elements per thread), column FFTs in
// place on strips of 64 columns (32 where H > 256), the radial reduce gathering Z(k) and Z(-k) from the workspace.  fft_lines and
// bin_partials are the same device functions in both forms.  The caller's workspace decides how many pairs go per chunk:
// pd_spectrum_ws_bytes asks for every pair of the call up to SP_WS_CAP = 256 MiB (127 pairs of 512 x 512), pd_spectrum_update runs as
// many chunks as the workspace it was given needs.
//
// Radial reduce: deterministic, no atomics.  One wave per bin walks the bin's cells in list order (lane-strided fp64 accumulators, then a
// fixed-order butterfly); per-pair partials [pair][3][nb] go to the workspace in fp64, and spectrum_fold_kernel adds them to the state
// pair by pair in index order.  The same inputs give the same bits.  No NaN masking: a NaN pixel makes its pair's bins NaN.
#include "axes.h"
#include "common.h"
#include "fft_lds.h"

namespace {

constexpr int SP_MAXM = 512;
constexpr int SP_LDS_ELEMS = 1024 * SP_PER_THREAD;             // 16384: elements of one workgroup's set of lines
constexpr int SP_LDS_LIMIT = 160 * 1024 - 512;
constexpr int64_t SP_WS_CAP = 256ll << 20;


// The three sums of bin b of one pair, by one wave: out[0], out[nb], out[2 nb].  z: the pair's transform, row pitch `pitch` (LDS or memory).
__device__ __forceinline__ void bin_partials(const float2* __restrict__ z, int pitch, int H, int W, const int* __restrict__ cell_order,
                                             const int* __restrict__ bin_start, int b, int nb, double s, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  double sp = 0.0, st = 0.0, sx = 0.0;
  const int i1 = bin_start[b + 1];
  for (int i = bin_start[b] + lane; i < i1; i += 64) {
    const int cell = cell_order[i];
    const int ky = cell / W, kx = cell - ky * W;
    const int my = ky ? H - ky : 0, mx = kx ? W - kx : 0;
    const float2 A = z[ky * pitch + kx], Bm = z[my * pitch + mx];          // Z(k), Z(-k)
    // P = (A + conj Bm) / 2, T = (A - conj Bm) / (2 i); sums and differences of two fp32 values are exact in fp64
    const double pr = 0.5 * ((double)A.x + (double)Bm.x), pi = 0.5 * ((double)A.y - (double)Bm.y);
    const double dr = (double)A.x - (double)Bm.x, di = (double)A.y + (double)Bm.y;
    const double tr = 0.5 * di, ti = -0.5 * dr;
    sp += pr * pr + pi * pi;
    st += tr * tr + ti * ti;
    sx += pr * tr + pi * ti;
  }
  sp = wave_sum_f64(sp), st = wave_sum_f64(st), sx = wave_sum_f64(sx);
  if (lane == 0) out[0] = s * sp, out[nb] = s * st, out[2 * nb] = s * sx;
}

// periodic Hann weight of index i on a side of n: 1/2 - 1/2 cos(2 pi i / n) = sin^2(pi i / n) (no cancellation near the edge)
__device__ __forceinline__ float hann(int i, int n) {
  const float s = sinpif((float)i / (float)n);
  return s * s;
}

struct SpPair {
  const float *p, *t;
};
// pair index ((m N + n) T + t) C + c -> the two planes
__device__ __forceinline__ SpPair pair_planes(const float* pred, const float* target, const Axes5& g, int64_t pred_stride_m,
                                              const Axes5& sp, const Axes5& st, int64_t pair) {
  const int64_t c = pair % g.c, t = (pair / g.c) % g.t, n = (pair / (g.c * g.t)) % g.n, m = pair / (g.c * g.t * g.n);
  return SpPair{pred + m * pred_stride_m + n * sp.n + t * sp.t + c * sp.c, target + n * st.n + t * st.t + c * st.c};
}

// rows [r0, r0 + nr) of the pair's two planes -> z[(r - r0) * pitch + w] = window * (p + i t)
__device__ __forceinline__ void load_rows(const SpPair& pp, const Axes5& sp, const Axes5& st, int H, int W, int r0, int nr,
                                          int window, float2* __restrict__ z, int pitch) {
  for (int i = threadIdx.x; i < nr * W; i += blockDim.x) {
    const int lr = i / W, w = i - lr * W;
    const int64_t h = r0 + lr;
    float a = pp.p[h * sp.h + w * sp.w], b = pp.t[h * st.h + w * st.w];
    if (window) {
      const float wn = hann((int)h, H) * hann(w, W);
      a *= wn, b *= wn;
    }
    z[lr * pitch + w] = make_float2(a, b);
  }
}

// LDS-resident form.  grid: the chunk's pairs; dynamic LDS: (H (W + 1) + max(H, W)) complex.
__global__ void __launch_bounds__(1024) spectrum_lds_kernel(const float* __restrict__ pred, const float* __restrict__ target, Axes5 g,
                                                            int64_t pred_stride_m, Axes5 sp, Axes5 st, int64_t pair0,
                                                            const int* __restrict__ cell_order, const int* __restrict__ bin_start,
                                                            int nb, int window, double* __restrict__ part) {
  extern __shared__ float2 sp_smem[];
  const int H = (int)g.h, W = (int)g.w, pitch = W + 1;
  float2* z = sp_smem;
  float2* tw = sp_smem + H * pitch;
  const SpPair pp = pair_planes(pred, target, g, pred_stride_m, sp, st, pair0 + blockIdx.x);
  load_rows(pp, sp, st, H, W, 0, H, window, z, pitch);
  fft_lines<false>(z, tw, H, W, pitch);
  fft_lines<true>(z, tw, W, H, pitch);
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const double s = 1.0 / ((double)H * (double)W);
  for (int b = wave; b < nb; b += nwaves)
    bin_partials(z, pitch, H, W, cell_order, bin_start, b, nb, s, part + (int64_t)blockIdx.x * 3 * nb + b);
}

// Strip form 1: row FFTs.  grid (pairs, row blocks of `rows`); zws[pair][h][w].
__global__ void __launch_bounds__(1024) spectrum_rows_kernel(const float* __restrict__ pred, const float* __restrict__ target, Axes5 g,
                                                             int64_t pred_stride_m, Axes5 sp, Axes5 st, int64_t pair0, int rows,
                                                             int window, float2* __restrict__ zws) {
  extern __shared__ float2 sp_smem[];
  const int H = (int)g.h, W = (int)g.w, pitch = W + 1;
  const int r0 = blockIdx.y * rows, nr = min(rows, H - r0);
  float2* z = sp_smem;
  float2* tw = sp_smem + rows * pitch;
  const SpPair pp = pair_planes(pred, target, g, pred_stride_m, sp, st, pair0 + blockIdx.x);
  load_rows(pp, sp, st, H, W, r0, nr, window, z, pitch);
  fft_lines<false>(z, tw, nr, W, pitch);
  float2* dst = zws + ((int64_t)blockIdx.x * H + r0) * W;
  for (int i = threadIdx.x; i < nr * W; i += blockDim.x) {
    const int lr = i / W, w = i - lr * W;
    dst[i] = z[lr * pitch + w];
  }
}

// Strip form 2: column FFTs in place on strips of `cs` columns.  grid (pairs, strips).
__global__ void __launch_bounds__(1024) spectrum_cols_kernel(float2* __restrict__ zws, int H, int W, int cs) {
  extern __shared__ float2 sp_smem[];
  const int pitch = cs + 1;
  const int c0 = blockIdx.y * cs, nc = min(cs, W - c0);
  float2* z = sp_smem;
  float2* tw = sp_smem + H * pitch;
  float2* src = zws + (int64_t)blockIdx.x * H * W + c0;
  for (int i = threadIdx.x; i < H * nc; i += blockDim.x) {
    const int h = i / nc, c = i - h * nc;
    z[h * pitch + c] = src[(int64_t)h * W + c];
  }
  fft_lines<true>(z, tw, nc, H, pitch);
  for (int i = threadIdx.x; i < H * nc; i += blockDim.x) {
    const int h = i / nc, c = i - h * nc;
    src[(int64_t)h * W + c] = z[h * pitch + c];
  }
}

// Strip form 3: the radial reduce over the workspace.  grid (pairs, ceil(nb / 4)), 4 waves: one bin each.
__global__ void __launch_bounds__(256) spectrum_reduce_kernel(const float2* __restrict__ zws, int H, int W, const int* __restrict__ cell_order,
                                                              const int* __restrict__ bin_start, int nb, double* __restrict__ part) {
  const int b = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (b >= nb) return;
  bin_partials(zws + (int64_t)blockIdx.x * H * W, W, H, W, cell_order, bin_start, b, nb, 1.0 / ((double)H * (double)W),
               part + (int64_t)blockIdx.x * 3 * nb + b);
}

// grid (ceil(nb / 256), T', 3): sums[k][tk][b] += the partials of the chunk's pairs of lead time tk (all pairs unless keep_seq), pair by
// pair in index order; thread (b = 0, k = 0) also adds the pairs to frames[tk].
__global__ void __launch_bounds__(256) spectrum_fold_kernel(const double* __restrict__ part, int64_t pair0, int np, int nb, int64_t T,
                                                            int64_t Cn, int keep_seq, double* __restrict__ sums,
                                                            long long* __restrict__ frames) {
  const int b = blockIdx.x * 256 + threadIdx.x, tk = blockIdx.y, k = blockIdx.z;
  if (b >= nb) return;
  const int64_t Tk = keep_seq ? T : 1;
  double a = 0.0;
  long long cnt = 0;
  for (int i = 0; i < np; ++i) {
    if (keep_seq && ((pair0 + i) / Cn) % T != tk) continue;
    a += part[((int64_t)i * 3 + k) * nb + b];
    ++cnt;
  }
  sums[((int64_t)k * Tk + tk) * nb + b] += a;
  if (b == 0 && k == 0) frames[tk] += cnt;
}

bool sp_geom(const int64_t* sizes, Axes5& g) { return read_axes(sizes, g) && sp_side_ok(g.h) && sp_side_ok(g.w); }

// pairs of the call; -1 when they do not fit a grid
int64_t sp_pairs(int M, const Axes5& g) {
  const double p = (double)M * (double)g.n * (double)g.t * (double)g.c;
  return p >= (double)(1 << 30) ? -1 : (int64_t)M * g.n * g.t * g.c;
}

bool sp_strip(const Axes5& g) { return g.h * g.w > SP_LDS_ELEMS; }
int sp_nb(const Axes5& g) { return (int)(std::max(g.h, g.w) / 2 + 1); }
int64_t sp_pair_bytes(const Axes5& g) { return 3ll * sp_nb(g) * 8 + (sp_strip(g) ? g.h * g.w * 8 : 0); }

}  // namespace

extern "C" int64_t pd_spectrum_ws_bytes(int M, const int64_t* sizes) {
  Axes5 g;
  if (M < 1 || M > SP_MAXM || !sp_geom(sizes, g)) return -1;
  const int64_t pairs = sp_pairs(M, g);
  if (pairs < 0) return -1;
  const int64_t per = sp_pair_bytes(g);
  return std::min(pairs * per, std::max(per, SP_WS_CAP / per * per));
}

extern "C" int pd_spectrum_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                                  const int64_t* target_strides, const int* cell_order, const int* bin_start, int nb, int window,
                                  int keep_seq, double* sums, long long* frames, void* ws, int64_t ws_bytes, pd_stream_t stream) {
  PD_CHECK_ARG(pred && target && sizes && pred_strides && target_strides && cell_order && bin_start && sums && frames && ws,
               "pd_spectrum_update: null pointer");
  PD_CHECK_ARG(M >= 1 && M <= SP_MAXM, "pd_spectrum_update: %d members (supported: 1 .. %d)", M, SP_MAXM);
  for (int i = 0; i < 5; ++i) PD_CHECK_ARG(sizes[i] >= 1, "pd_spectrum_update: axis %d has size %lld", i, (long long)sizes[i]);
  for (int i = 2; i < 4; ++i)
    PD_CHECK_ARG(sp_side_ok(sizes[i]), "pd_spectrum_update: side %lld of the %lld x %lld frames is not supported (2^a or 3 * 2^a, %d .. %d)",
                 (long long)sizes[i], (long long)sizes[2], (long long)sizes[3], SP_MIN_SIDE, SP_MAX_SIDE);
  PD_CHECK_ARG(window == 0 || window == 1, "pd_spectrum_update: window %d (0: none, 1: hann)", window);
  Axes5 g;
  PD_CHECK_ARG(sp_geom(sizes, g), "pd_spectrum_update: bad sizes");
  const int64_t pairs = sp_pairs(M, g);
  PD_CHECK_ARG(pairs > 0, "pd_spectrum_update: too many frames in one update");
  PD_CHECK_ARG(nb == sp_nb(g), "pd_spectrum_update: %d bins for %lld x %lld frames (max(H, W) / 2 + 1 = %d)", nb, (long long)g.h,
               (long long)g.w, sp_nb(g));
  const int64_t per = sp_pair_bytes(g);
  PD_CHECK_ARG(ws_bytes >= per, "pd_spectrum_update: workspace of %lld bytes < %lld (one pair)", (long long)ws_bytes, (long long)per);
  PD_CHECK_ARG(((uintptr_t)ws & 7) == 0, "pd_spectrum_update: workspace not 8-byte aligned");
  const int64_t chunk = std::min(pairs, ws_bytes / per);
  const int H = (int)g.h, W = (int)g.w;
  const bool strip = sp_strip(g);
  const Axes5 sp = read_strides(pred_strides + 1), st = read_strides(target_strides);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;                          // [chunk][3][nb]
  float2* zws = (float2*)(part + chunk * 3 * nb);      // [chunk][H][W], strip form only
  static bool lds_set[3][PD_MAX_DEVICES];
  if (strip) {
    if (int rc = pd_raise_lds("pd_spectrum_update", (const void*)spectrum_rows_kernel, SP_LDS_LIMIT, lds_set[1])) return rc;
    if (int rc = pd_raise_lds("pd_spectrum_update", (const void*)spectrum_cols_kernel, SP_LDS_LIMIT, lds_set[2])) return rc;
  } else if (int rc = pd_raise_lds("pd_spectrum_update", (const void*)spectrum_lds_kernel, SP_LDS_LIMIT, lds_set[0])) {
    return rc;
  }
  for (int64_t p0 = 0; p0 < pairs; p0 += chunk) {
    const int np = (int)std::min(chunk, pairs - p0);
    if (!strip) {
      const int threads = H * W <= 256 * SP_PER_THREAD ? 256 : 1024;
      const size_t lds = sizeof(float2) * ((size_t)H * (W + 1) + std::max(H, W));
      hipLaunchKernelGGL(spectrum_lds_kernel, dim3(np), dim3(threads), lds, s, pred, target, g, pred_strides[0], sp, st, p0, cell_order,
                         bin_start, nb, window, part);
      PD_CHECK_LAUNCH();
    } else {
      // rows per workgroup: what 1024 threads hold in one stage (15 elements each where the row has a radix-3 stage)
      const int rows = std::min(H, (W % 3 == 0 ? 1024 * (SP_PER_THREAD / 3) * 3 : SP_LDS_ELEMS) / W), cs = H > 256 ? 32 : 64;
      const size_t lds_r = sizeof(float2) * ((size_t)rows * (W + 1) + W), lds_c = sizeof(float2) * ((size_t)H * (cs + 1) + H);
      hipLaunchKernelGGL(spectrum_rows_kernel, dim3(np, (H + rows - 1) / rows), dim3(1024), lds_r, s, pred, target, g, pred_strides[0], sp,
                         st, p0, rows, window, zws);
      PD_CHECK_LAUNCH();
      hipLaunchKernelGGL(spectrum_cols_kernel, dim3(np, (W + cs - 1) / cs), dim3(1024), lds_c, s, zws, H, W, cs);
      PD_CHECK_LAUNCH();
      hipLaunchKernelGGL(spectrum_reduce_kernel, dim3(np, (nb + 3) / 4), dim3(256), 0, s, (const float2*)zws, H, W, cell_order, bin_start,
                         nb, part);
      PD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(spectrum_fold_kernel, dim3((nb + 255) / 256, (unsigned)(keep_seq ? g.t : 1), 3), dim3(256), 0, s,
                       (const double*)part, p0, np, nb, g.t, g.c, keep_seq, sums, frames);
    PD_CHECK_LAUNCH();
  }
  return PD_OK;
}
