// MX (OCP microscaling) e4m3 operands: the stand-alone quantiser and the entry point of the block-scaled implicit GEMM (the kernel is
// the MX instantiation of igemm256_kernel, igemm256.hip).  bfloat16 build only: an MX launch has no 16-bit operand.
#include <algorithm>
#include "mx_quant.h"

namespace PD_NS {

bool pd_igemm_operand_extents(pd_igemm_args& a);       // igemm.hip
int pd_igemm_vec_epilogue(const pd_igemm_args& a);
bool pd_igemm256_supported(const pd_igemm_args& a, int kind);
int pd_igemm256_ksplit(const pd_igemm_args& a, int kind);
int pd_igemm256_launch_mx(const pd_igemm_args& a, const pd_mx_operands& m, int kind, hipStream_t s);

// one thread per four elements of a padded row; the 8 threads of a block sit in 8 consecutive lanes (ld % 32 == 0)
__global__ void __launch_bounds__(256) quantize_mx_kernel(const float* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ scales,
                                                          int64_t rows, int K, int ld_x, int ld) {
  const int cvs = ld >> 2;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= rows * cvs) return;                    // (whole blocks of 8 lanes leave together: rows * cvs is a multiple of 8)
  const int64_t row = id / cvs;
  const int c = (int)(id - row * cvs) * 4;
  float y[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < K) {
    const float4 v = *(const float4*)(x + row * (int64_t)ld_x + c);
    y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
  }
  int sb;
  const uint32_t w = mx_quantize4(y, sb);
  *(uint32_t*)(q + row * (int64_t)ld + c) = w;
  if ((c & 31) == 0) scales[row * (int64_t)(ld >> 5) + (c >> 5)] = (uint8_t)sb;
}

extern "C" int pd_quantize_mx(const float* x, uint8_t* q, uint8_t* scales, int64_t rows, int K, int ld_x, int ld, pd_stream_t stream) {
  PD_CHECK_ARG(x && q && scales, "pd_quantize_mx: null pointer");
  PD_CHECK_ARG(K > 0 && (K & 31) == 0, "pd_quantize_mx: K=%d must be a positive multiple of 32 (one scale per 32 elements)", K);
  PD_CHECK_ARG(ld >= K && (ld & 31) == 0 && ld_x >= K && (ld_x & 3) == 0, "pd_quantize_mx: ld=%d must be a multiple of 32 and >= K, ld_x=%d a multiple of 4 and >= K", ld, ld_x);
  PD_CHECK_ARG((((uintptr_t)x) & 15) == 0 && (((uintptr_t)q) & 3) == 0, "pd_quantize_mx: x must be 16 B aligned, q 4 B aligned");
  if (rows <= 0) return PD_OK;
  const int64_t n = rows * (ld >> 2);
  PD_CHECK_ARG((n + 255) / 256 < 0x7fffffffll, "pd_quantize_mx: too many rows");
  hipLaunchKernelGGL(quantize_mx_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, q, scales, rows, K, ld_x, ld);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int pd_igemm_mx(const pd_igemm_args* pa, const pd_mx_operands* pm, pd_stream_t stream) {
  PD_CHECK_ARG(pa != nullptr && pm != nullptr, "pd_igemm_mx: null args");
  pd_igemm_args a = *pa;
  const pd_mx_operands& m = *pm;
  PD_CHECK_ARG(a.A && a.W && m.a_scales && m.w_scales, "pd_igemm_mx: A / W / scales null");
  PD_CHECK_ARG(!a.fp8 && !a.split && !a.w_fold && !a.operand && !a.tile && !a.out_fp8_log2 && !a.A_lo && !a.W_lo && !a.out_bf16_lo && a.nbatch <= 1,
               "pd_igemm_mx: fp8 / split / w_fold / operand / tile / out_fp8_log2 must be 0, no low halves, no batch");
  PD_CHECK_ARG(a.M > 0 && a.N > 0 && a.taps > 0, "pd_igemm_mx: bad M/N/taps (%d,%d,%d)", a.M, a.N, a.taps);
  PD_CHECK_ARG(a.Cin > 0 && (a.Cin & 127) == 0 && (a.lda & 127) == 0 && (a.ldw & 127) == 0 && a.lda >= a.Cin && a.ldw >= a.Cin,
               "pd_igemm_mx: Cin=%d, lda=%d, ldw=%d must be multiples of 128 (K-tiles of four blocks) with lda, ldw >= Cin", a.Cin, a.lda, a.ldw);
  PD_CHECK_ARG(m.ld_a_scales * 32 == a.lda && m.ld_w_scales * 32 == a.ldw, "pd_igemm_mx: ld_a_scales / ld_w_scales must be lda / 32, ldw / 32");
  PD_CHECK_ARG((((uintptr_t)m.a_scales | (uintptr_t)m.w_scales) & 3) == 0 && (m.w_scale_tap_stride & 3) == 0 && m.w_scale_tap_stride >= 0,
               "pd_igemm_mx: the scale arrays and the tap stride of w_scales must be 4 B aligned");
  PD_CHECK_ARG(a.taps == a.KT * a.KH * a.KW, "pd_igemm_mx: taps != KT*KH*KW");
  PD_CHECK_ARG((int64_t)a.B * a.To * a.Ho * a.Wo == a.M, "pd_igemm_mx: M != B*To*Ho*Wo");
  PD_CHECK_ARG(a.ut == 1 && a.uh == 1 && a.uw == 1 && a.vT <= 0 && a.vH <= 0 && a.vW <= 0, "pd_igemm_mx: no up-sampling");
  PD_CHECK_ARG(!a.rowvec || a.rows_per_sample > 0, "pd_igemm_mx: rowvec needs rows_per_sample");
  PD_CHECK_ARG(a.out_f32 || a.out_bf16, "pd_igemm_mx: no output");
  const bool pointwise = a.taps == 1 && a.st == 1 && a.sh == 1 && a.sw == 1 && a.pt == 0 && a.ph == 0 && a.pw == 0 && a.Ti == a.To &&
                         a.Hi == a.Ho && a.Wi == a.Wo;
  const int kind = pointwise ? 0 : 2;
  a.fp8 = 1;                        // (e4m3 payload: the K-tile count and the operand extents of the shared helpers)
  PD_CHECK_ARG(pd_igemm_operand_extents(a) && (int64_t)(a.taps - 1) * m.w_scale_tap_stride < 0x7fffffffll,
               "pd_igemm_mx: operand larger than a 4 GiB buffer descriptor");
  a.vec_epilogue = pd_igemm_vec_epilogue(a);
  if (!pd_igemm256_supported(a, kind)) {
    pd_set_error("pd_igemm_mx: MX operands are built for row-wise linear layers and stride-1, un-upsampled convolutions only");
    return PD_ERR_UNSUPPORTED;
  }
  // small grids: K-slices as extra workgroups, as the unit-scale e4m3 form.  debug_flags bit 128 (tests; pd_igemm ignores it): two to
  // four slices whenever a workspace is given, whatever the grid
  a.ksplit = 1;
  int ks = a.disable_256 ? 0 : pd_igemm256_ksplit(a, kind);
  if (ks < 2 && (a.debug_flags & 128) && a.splitk_ws && (a.N & 3) == 0) {
    const int64_t nk = (int64_t)a.taps * (a.Cin >> 7);
    ks = (int)std::min<int64_t>(std::min<int64_t>(nk, 4), a.splitk_ws_elems / ((int64_t)a.M * a.N));
  }
  if (ks >= 2) a.ksplit = ks;
  return pd_igemm256_launch_mx(a, m, kind, (hipStream_t)stream);
}

}  // namespace PD_NS
