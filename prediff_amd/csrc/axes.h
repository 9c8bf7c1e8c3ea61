// The N, T, H, W, C plumbing of the score kernels (ensemble_score.hip, frame_score.hip, spectrum.hip): every operand is addressed
// through the sizes and element strides of these five axes, which the host passes as int64[5] (an axis the layout does not name has
// size 1, stride 0).  What a file derives from the sizes (pooled sides, tile counts, side rules) stays in that file.
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
