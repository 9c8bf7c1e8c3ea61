// The LDS-resident 1-D FFT core shared by spectrum.hip and steps.hip (the header of spectrum.hip describes it): Stockham autosort in
// LDS, radix-4 stages, one radix-2 stage when log2 is odd, one radix-3 stage last.  Line lengths 2^a or 3 2^a.  A stage is
// read - barrier - write over the SAME buffer, a thread holds at most SP_PER_THREAD elements of it in registers (compile-time indexed: no
// scratch).  The transform is the forward one, exp(-2 pi i ...); an inverse is the forward one on conjugated data, scaled by the caller.
#pragma once
#include "common.h"

namespace {

constexpr int SP_PER_THREAD = 16;                              // complex elements a thread holds during one stage
constexpr int SP_MIN_SIDE = 8, SP_MAX_SIDE = 512;              // frame sides of the 2-D users (host check: sp_side_ok)

// a side the 2-D transforms take: 2^a or 3 2^a within the limits
inline bool sp_side_ok(int64_t n) {
  if (n < SP_MIN_SIDE || n > SP_MAX_SIDE) return false;
  if (n % 3 == 0) n /= 3;
  return (n & (n - 1)) == 0;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmuli_neg(float2 a) { return make_float2(a.y, -a.x); }       // a * (-i)

// forward R-point DFT of v (kernel exp(-2 pi i r q / R)), in registers
template <int R>
__device__ __forceinline__ void butterfly(float2 (&v)[R]) {
  if constexpr (R == 2) {
    const float2 a = v[0], b = v[1];
    v[0] = cadd(a, b), v[1] = csub(a, b);
  } else if constexpr (R == 4) {
    const float2 t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]), t2 = cadd(v[1], v[3]), t3 = cmuli_neg(csub(v[1], v[3]));
    v[0] = cadd(t0, t2), v[1] = cadd(t1, t3), v[2] = csub(t0, t2), v[3] = csub(t1, t3);
  } else {
    const float2 s = cadd(v[1], v[2]), d0 = cmuli_neg(csub(v[1], v[2]));
    const float2 d = make_float2(0.86602540378443864676f * d0.x, 0.86602540378443864676f * d0.y);
    const float2 m = make_float2(fmaf(-0.5f, s.x, v[0].x), fmaf(-0.5f, s.y, v[0].y));
    v[0] = cadd(v[0], s), v[1] = cadd(m, d), v[2] = csub(m, d);
  }
}

// tw[m] = exp(-2 pi i m / N), m < N.  The angle is (q + r / N) quarter turns with q = 4 m / N and r = 4 m - q N in integers:
// sincospif sees 0.5 r / N in [0, 0.5) (one fp32 rounding of a quotient below a half), the quadrant is a sign / swap.
__device__ __forceinline__ void build_twiddles(float2* __restrict__ tw, int N) {
  for (int m = threadIdx.x; m < N; m += blockDim.x) {
    const int q = 4 * m / N, r = 4 * m - q * N;
    float s, c;
    sincospif(0.5f * ((float)r / (float)N), &s, &c);
    const float co = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
    const float si = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    tw[m] = make_float2(co, -si);
  }
}

// One radix-R Stockham stage over nl lines of length N in LDS, in place (read - barrier - write).  Element e of line l is at
// buf[COLS ? e * pitch + l : l * pitch + e].  Work item w = (line, butterfly j < N / R); COLS: lines fastest (adjacent lanes, adjacent
// columns), else j fastest (adjacent lanes, adjacent elements of a row).  Ns: length of the sub-transforms done so far (a power of two).
// Requires nl * N <= blockDim.x * (SP_PER_THREAD / R) * R: 16 elements per thread, 15 in the radix-3 stage.
template <int R, bool COLS>
__device__ __forceinline__ void fft_stage(float2* __restrict__ buf, const float2* __restrict__ tw, int nl, int N, int pitch, int Ns) {
  constexpr int B = SP_PER_THREAD / R;
  const int npl = N / R, total = nl * npl, tstep = N / (Ns * R);
  float2 v[B][R];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int w = threadIdx.x + b * blockDim.x;
    if (w < total) {
      const int line = COLS ? w % nl : w / npl, j = COLS ? w / nl : w % npl;
      const int k = j & (Ns - 1);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int e = j + r * npl;
        v[b][r] = buf[COLS ? e * pitch + line : line * pitch + e];
      }
#pragma unroll
      for (int r = 1; r < R; ++r) v[b][r] = cmul(v[b][r], tw[r * k * tstep]);
      butterfly<R>(v[b]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int w = threadIdx.x + b * blockDim.x;
    if (w < total) {
      const int line = COLS ? w % nl : w / npl, j = COLS ? w / nl : w % npl;
      const int k = j & (Ns - 1), j0 = (j - k) * R + k;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int e = j0 + r * Ns;
        buf[COLS ? e * pitch + line : line * pitch + e] = v[b][r];
      }
    }
  }
  __syncthreads();
}

// forward FFT of nl lines of length N (2^a or 3 2^a) in LDS; tw: N complex of LDS.  Every thread of the workgroup calls it.
template <bool COLS>
__device__ __forceinline__ void fft_lines(float2* __restrict__ buf, float2* __restrict__ tw, int nl, int N, int pitch) {
  __syncthreads();                                     // the last user of tw / writer of buf is done
  build_twiddles(tw, N);
  __syncthreads();
  const bool three = N % 3 == 0;
  const int a = __ffs(three ? N / 3 : N) - 1;
  int Ns = 1;
  for (int i = 0; i < a / 2; ++i, Ns *= 4) fft_stage<4, COLS>(buf, tw, nl, N, pitch, Ns);
  if (a & 1) {
    fft_stage<2, COLS>(buf, tw, nl, N, pitch, Ns);
    Ns *= 2;
  }
  if (three) fft_stage<3, COLS>(buf, tw, nl, N, pitch, Ns);
}

}  // namespace
