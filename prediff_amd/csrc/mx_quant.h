// MX (OCP microscaling) e4m3 quantisation of one 32-element block, shared by pd_quantize_mx (mx.hip) and the two norm producers
// (norm.hip).  DESIGN.md section 7 states the format; tests/_mx_ref.py restates it in numpy.
#pragma once
#include "common.h"

// E8M0 scale byte of a block from its amax (>= 0, finite): 127 + e with e = floor(log2(amax)) - 8 (8 = emax of e4m3), one more where
// amax * 2^-e would lie above 448 = 1.75 * 2^8, the largest e4m3 value (so no payload saturates), clamped below at 0.  An all-zero block
// (and any amax below 2^-119) gets byte 0, the smallest scale.  The exponent field of amax IS floor(log2(amax)) + 127.
__device__ __forceinline__ int mx_scale_byte(float amax) {
  const uint32_t u = __float_as_uint(amax);
  const int e = (int)(u >> 23) - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  return e > 0 ? e : 0;
}
// 2^(127 - byte): what a value is multiplied by before it is rounded to e4m3 (byte <= 247: a normal fp32)
__device__ __forceinline__ float mx_inv_scale(int byte) { return __uint_as_float((uint32_t)(254 - byte) << 23); }

// max over the 8 consecutive lanes (aligned at 8) that hold one 32-element block, four elements each
__device__ __forceinline__ float mx_block_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64));
  v = fmaxf(v, __shfl_xor(v, 2, 64));
  return fmaxf(v, __shfl_xor(v, 4, 64));
}

// four fp32 -> four OCP e4m3 bytes of y * scale in one dword, saturating at +-448 (v_cvt_pk_fp8_f32 rounds to nearest even): the one e4m3
// packer of the norm producers, unit-scale (norm.hip) and MX (below)
__device__ __forceinline__ uint32_t pack_e4m3x4(const float (&y)[4], float scale) {
  float q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = fminf(fmaxf(y[k] * scale, -448.f), 448.f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], w, true);
  return (uint32_t)w;
}

// this lane's four elements of a block -> four payload bytes (round to nearest even; the clamp never binds on finite input) and the block's
// scale byte
__device__ __forceinline__ uint32_t mx_quantize4(const float (&y)[4], int& scale_byte) {
  const float amax = mx_block_max(fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3]))));
  scale_byte = mx_scale_byte(amax);
  return pack_e4m3x4(y, mx_inv_scale(scale_byte));
}
