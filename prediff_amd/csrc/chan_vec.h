// Channels-last fp32 passes that move whole channel vectors (tile_blend.hip, rollout.hip): one thread per output element, which is a
// float4 of channels when C % 4 == 0 and every buffer is 16-byte aligned and one float otherwise; 256 threads, grid-stride loop.
#pragma once
#include "common.h"

static inline unsigned grid_for(int64_t n) { return (unsigned)min((int64_t)8192, (n + 255) / 256); }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int V> struct vec_of;
template <> struct vec_of<1> { typedef float type; };
template <> struct vec_of<4> { typedef float4 type; };

__device__ __forceinline__ void vzero(float& v) { v = 0.f; }
__device__ __forceinline__ void vzero(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
