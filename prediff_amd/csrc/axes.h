// The N, T, H, W, C plumbing of the score kernels (ensemble_score.hip, frame_score.hip, spectrum.hip, distances.hip, scales.hip): every
// operand is addressed through the sizes and element strides of these five axes, which the host passes as int64[5] (an axis the layout
// does not name has size 1, stride 0).  What a file derives from the sizes (pooled sides, tile counts, side rules) stays in that file;
// the extent of a strided operand and the aliasing test of the host checks are here.
#pragma once
#include <stdint.h>

struct Axes5 {
  int64_t n, t, h, w, c;               // sizes or element strides
};

// sizes: all five present and >= 1
inline bool read_axes(const int64_t* sizes, Axes5& a) {
  if (!sizes) return false;
  for (int i = 0; i < 5; ++i)
    if (sizes[i] < 1) return false;
  a = Axes5{sizes[0], sizes[1], sizes[2], sizes[3], sizes[4]};
  return true;
}

inline Axes5 read_strides(const int64_t* s) { return Axes5{s[0], s[1], s[2], s[3], s[4]}; }

// bytes from the base to the end of the last fp32 element that `lead` leading indices of stride s_lead and sizes / strides (n axes)
// address; -1: a negative stride
inline int64_t axes_span(const int64_t* sizes, const int64_t* strides, int n, int64_t lead, int64_t s_lead) {
  int64_t last = 0;
  if (s_lead < 0) return -1;
  last += (lead - 1) * s_lead;
  for (int i = 0; i < n; ++i) {
    if (strides[i] < 0) return -1;
    last += (sizes[i] - 1) * strides[i];
  }
  return (last + 1) * (int64_t)sizeof(float);
}

inline bool bytes_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const char *pa = (const char*)a, *pb = (const char*)b;
  return pa < pb + b_bytes && pb < pa + a_bytes;
}
