// The one bilinear sampling rule of the extrapolation kernels (pd_advect in extrapolation.hip; steps.hip and anvil.hip through
// frame_lds.h, which rely on sampling exactly as pd_advect does).
#pragma once
#include "common.h"

constexpr float BIL_FAR = 1048576.f;                           // 2^20

// I(cy, cx) of the H x W frame I, bilinear from floor.  A tap outside the frame reads `fill`; a coordinate that is not finite or lies
// further than 2^20 from the frame gives `fill` before any integer is made of it (the motion may be the caller's).
__device__ __forceinline__ float bil_fill(const float* __restrict__ I, int H, int W, float cy, float cx, float fill) {
  float r = fill;
  // false for a NaN
  if (cy >= -BIL_FAR && cy <= (float)(H - 1) + BIL_FAR && cx >= -BIL_FAR && cx <= (float)(W - 1) + BIL_FAR) {
    const float y0f = floorf(cy), x0f = floorf(cx);
    const float fy = cy - y0f, fx = cx - x0f;
    const int y0 = (int)y0f, x0 = (int)x0f;
    const bool r0 = y0 >= 0 && y0 < H, r1 = y0 + 1 >= 0 && y0 + 1 < H;
    const bool c0 = x0 >= 0 && x0 < W, c1 = x0 + 1 >= 0 && x0 + 1 < W;
    const float i00 = r0 && c0 ? I[y0 * W + x0] : fill;
    const float i01 = r0 && c1 ? I[y0 * W + x0 + 1] : fill;
    const float i10 = r1 && c0 ? I[(y0 + 1) * W + x0] : fill;
    const float i11 = r1 && c1 ? I[(y0 + 1) * W + x0 + 1] : fill;
    const float top = i00 + fx * (i01 - i00);
    const float bot = i10 + fx * (i11 - i10);
    r = top + fy * (bot - top);
  }
  return r;
}
