// Epilogue shared by the pd_igemm kernels: a wave's fp32 accumulator slab (WM rows x WNS columns, row major in LDS) ->
// alpha, bias, per-sample row vector (timestep embedding), activation, gate multiply, fp32 residual add -> coalesced
// 16 B row segments of the fp32 and/or bf16 (hi[/lo]) outputs.
#pragma once
#include <type_traits>
#include "common.h"

// The row loop is instantiated per (columns-per-lane, activation, operand presence) so that the hot call sites get
// straight-line code; tag value 2 = "decide at run time" (generic instantiation).
//   CW columns per lane: 8 when only bf16 is stored (16 B stores: the 8 B/lane form is store-issue bound), else 4.
template <int WM, int WNS, int CW, int ACT, int RV, int MU, int RS, int OF, int OB, int OL>
__device__ __forceinline__ void igemm_epilogue_rows(const pd_igemm_args& p, const float* sC, int lane, int m_base, int m_end, int n_base,
                                                    float* outf, pd_bf16* outb, pd_bf16* outbl, const float* res) {
  auto on = [](int tag, bool rt) { return tag == 2 ? rt : (tag == 1); };
  constexpr int LPR = WNS / CW;                    // lanes per row
  constexpr int RPP = 64 / LPR;                    // rows per pass
  const int c0 = (lane % LPR) * CW;
  const int n = n_base + c0;
  const bool vec = p.vec_epilogue && (n + CW - 1 < p.N);
  const bool has_rv = on(RV, p.rowvec != nullptr), has_mu = on(MU, p.mul != nullptr), has_rs = on(RS, res != nullptr);
  const bool has_of = on(OF, outf != nullptr), has_ob = on(OB, outb != nullptr), has_ol = on(OL, outbl != nullptr);
  const bool has_rt = RV == 2 && p.rowtab != nullptr;      // per-row additive table: the run-time (generic) instantiations only
  const int act = ACT >= 0 ? ACT : ((p.debug_flags & 4) ? 0 : p.act);
  float bias_v[CW];
#pragma unroll
  for (int e = 0; e < CW; ++e) bias_v[e] = (p.bias && n + e < p.N) ? p.bias[n + e] : 0.f;
  if (n >= p.N || (p.debug_flags & 2)) return;
#pragma unroll 1
  for (int pass = 0; pass < WM / RPP; ++pass) {
    const int row = pass * RPP + lane / LPR;
    const int m = m_base + row;
    if (m >= m_end) continue;
    float v[CW];
#pragma unroll
    for (int q = 0; q < CW / 4; ++q) {
      const float4 a4 = *(const float4*)(sC + row * WNS + c0 + 4 * q);
      v[4 * q] = a4.x; v[4 * q + 1] = a4.y; v[4 * q + 2] = a4.z; v[4 * q + 3] = a4.w;
    }
    const float* rv = has_rv ? p.rowvec + (int64_t)(m / p.rows_per_sample) * p.ld_rowvec + n : nullptr;
    const float* mu = has_mu ? p.mul + (int64_t)m * p.ld_mul + n : nullptr;
    const float* rs = has_rs ? res + (int64_t)(p.res_period ? m % p.res_period : m) * p.ld_res + n : nullptr;
    const float* rt = has_rt ? p.rowtab + (int64_t)(m % p.rowtab_rows) * p.N + n : nullptr;
    if (vec) {
#pragma unroll
      for (int e = 0; e < CW; ++e) v[e] = v[e] * p.alpha + bias_v[e];
      if (has_rv) {
#pragma unroll
        for (int q = 0; q < CW / 4; ++q) { const float4 t4 = *(const float4*)(rv + 4 * q); v[4 * q] += t4.x; v[4 * q + 1] += t4.y; v[4 * q + 2] += t4.z; v[4 * q + 3] += t4.w; }
      }
      if (act != 0) {
        // a 16-bit-only producer (FFN-1 of the single-pass engines; compile-time in the hot instantiation, the same rule at run time in
        // the generic ones): the 9-instruction sigmoid-form GELU, 2.5e-5 from the erf form and rounded to 16 bits right below; an fp32
        // or hi/lo output (the fp32-class engine) keeps act_apply's erf form
        const bool only16 = (ACT == PD_ACT_GELU && OL == 0 && OF == 0) || (has_ob && !has_ol && !has_of);
#pragma unroll
        for (int e = 0; e < CW; ++e) v[e] = only16 ? act_apply16(v[e], act) : act_apply(v[e], act);
      }
      if (has_mu) {
#pragma unroll
        for (int q = 0; q < CW / 4; ++q) { const float4 t4 = *(const float4*)(mu + 4 * q); v[4 * q] *= t4.x; v[4 * q + 1] *= t4.y; v[4 * q + 2] *= t4.z; v[4 * q + 3] *= t4.w; }
      }
      if (has_rs) {
#pragma unroll
        for (int q = 0; q < CW / 4; ++q) { const float4 t4 = *(const float4*)(rs + 4 * q); v[4 * q] += t4.x; v[4 * q + 1] += t4.y; v[4 * q + 2] += t4.z; v[4 * q + 3] += t4.w; }
      }
      if (has_rt) {
#pragma unroll
        for (int q = 0; q < CW / 4; ++q) { const float4 t4 = *(const float4*)(rt + 4 * q); v[4 * q] += t4.x; v[4 * q + 1] += t4.y; v[4 * q + 2] += t4.z; v[4 * q + 3] += t4.w; }
      }
      if (has_of) {
#pragma unroll
        for (int q = 0; q < CW / 4; ++q)
          *(float4*)(outf + (int64_t)m * p.ld_out + n + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
      }
      if (CW == 8 && has_ob && p.out_fp8_log2 > 0) {
        // e4m3 bytes, value * 2^k, round to nearest even, saturating: the A operand of a following fp8 launch
        const float f8s = __builtin_amdgcn_ldexpf(1.0f, p.out_fp8_log2);
        int w[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          float y[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) y[k] = fminf(fmaxf(v[4 * q + k] * f8s, -448.f), 448.f);
          w[q] = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
          w[q] = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w[q], true);
        }
        *(uint2*)((uint8_t*)outb + (int64_t)m * p.ld_outb + n) = make_uint2((uint32_t)w[0], (uint32_t)w[1]);
      } else if (has_ob) {
        uint32_t hi[CW / 2], lo[CW / 2];
#pragma unroll
        for (int e = 0; e < CW / 2; ++e) {
          if (has_ol) {
            uint16_t h0, l0, h1, l1;
            f2bf_split(v[2 * e], h0, l0);
            f2bf_split(v[2 * e + 1], h1, l1);
            hi[e] = h0 | ((uint32_t)h1 << 16);
            lo[e] = l0 | ((uint32_t)l1 << 16);
          } else {
            hi[e] = pack_op2(v[2 * e], v[2 * e + 1]);
          }
        }
        if constexpr (CW == 8) {
          *(uint4*)(outb + (int64_t)m * p.ld_outb + n) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
          if (has_ol) *(uint4*)(outbl + (int64_t)m * p.ld_outb + n) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        } else {
          *(uint2*)(outb + (int64_t)m * p.ld_outb + n) = make_uint2(hi[0], hi[1]);
          if (has_ol) *(uint2*)(outbl + (int64_t)m * p.ld_outb + n) = make_uint2(lo[0], lo[1]);
        }
      }
    } else {
      for (int e = 0; e < CW; ++e) {
        if (n + e >= p.N) break;
        float x = v[e] * p.alpha + bias_v[e];
        if (rv) x += rv[e];
        x = (has_ob && !has_ol && !has_of) ? act_apply16(x, act) : act_apply(x, act);
        if (mu) x *= mu[e];
        if (rs) x += rs[e];
        if (rt) x += rt[e];
        if (has_of) outf[(int64_t)m * p.ld_out + n + e] = x;
        if (has_ob) {
          uint16_t h, l;
          f2bf_split(x, h, l);
          outb[(int64_t)m * p.ld_outb + n + e] = h;
          if (has_ol) outbl[(int64_t)m * p.ld_outb + n + e] = l;
        }
      }
    }
  }
}

// ---- the fp32 residual-stream writers, pipelined (the default; debug_flags bit 32 keeps the serial loop above for A/B runs) ----
// The serial loop makes one HBM round trip per pass: vmcnt counts loads and stores alike and retires in order, so the wait for a pass's
// operand load also waits for the previous pass's store.  Here a slab's passes go in batches of R: the operand loads of batch b + 1 are
// issued before the LDS reads, the arithmetic and the R stores of batch b, so the counted wait of a load covers at most the stores of the
// batch before the previous one, and a wave keeps up to 2 R loads + R stores in flight (< 63, the vmcnt field).  Per element the
// operations and their order are those of the serial loop (fma(acc, alpha, bias), then + rowvec or + residual): the same bits.
//  - A lane stores exactly the 16 B it loaded, in the pass it loaded them for: an in-place launch (residual == out_f32) stays correct.
//  - Rows >= m_end are not stored; their operand loads read row m_end - 1 instead (no branch round a load: it would serialise the
//    batch).  All WM rows of the slab are read, written by the caller or not: sC .. sC + WM * WNS must be the wave's own LDS.
//  - m % res_period only when res_period != 0; the row vector once per slab when the slab lies inside one sample (UNI).
#ifndef PD_EPI_R
// Passes per batch.  4, 8 and 16 were built and measured (profiles/igemm_epilogue_ab.txt): none has scratch, and they time the same, in
// the isolated Conv3d launches and in the headline -- with 4 the epilogue-only launch already moves its bytes at the HBM rate -- so the
// one with the fewest registers stays: a wave has 8 loads + 4 stores of 1 KB in flight.  (-DPD_EPI_R=n builds another for A/B runs.)
#define PD_EPI_R 4
#endif
//  - TB: the per-row additive table (row m % rowtab_rows of p.rowtab, N columns; with the residual form only) is a second operand stream,
//    loaded with the residual's and added after it: ((acc * alpha + bias) + residual) + table, the order of a pd_add_rowtable launch
//    behind the convolution.
template <int WM, int WNS, int RV, int RS, int R, bool TB = false>
__device__ __forceinline__ void igemm_epilogue_rows_f32(const pd_igemm_args& p, const float* sC, int lane, int m_base, int m_end, int n_base,
                                                        float* outf, const float* res) {
  static_assert(RV + RS == 1, "one global operand: the per-sample row vector or the residual");
  constexpr int LPR = WNS / 4;                     // lanes per row
  constexpr int RPP = 64 / LPR;                    // rows per pass
  constexpr int NP = WM / RPP;                     // passes per slab
  static_assert(NP % R == 0 && (TB ? 5 : 3) * R < 63, "whole batches; loads + stores in flight fit the vmcnt field");
  static_assert(!TB || RS, "the row table goes with the residual form");
  constexpr int NB = NP / R;
  if (m_base >= m_end) return;
  const int c0 = (lane % LPR) * 4;
  const int row0 = lane / LPR;
  const int n = n_base + c0;
  const int m_last = m_end - 1;
  float bias_v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) bias_v[e] = p.bias ? p.bias[n + e] : 0.f;
  const float alpha = p.alpha;
  auto run = [&](auto uni, auto full) {
    constexpr bool UNI = decltype(uni)::value;       // one row vector for the whole slab
    constexpr bool FULL = decltype(full)::value;     // every row of the slab is stored: no lane predicate round the stores
    float4 rv0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (UNI) rv0 = *(const float4*)(p.rowvec + (int64_t)(m_base / p.rows_per_sample) * p.ld_rowvec + n);
    auto issue = [&](int b, float4(&d)[R], float4(&dt)[TB ? R : 1]) {
      if (UNI) return;
      int src[R];
#pragma unroll
      for (int r = 0; r < R; ++r) src[r] = FULL ? m_base + (b * R + r) * RPP + row0 : min(m_base + (b * R + r) * RPP + row0, m_last);
      if constexpr (TB) {
#pragma unroll
        for (int r = 0; r < R; ++r) dt[r] = *(const float4*)(p.rowtab + (int64_t)(src[r] % p.rowtab_rows) * p.N + n);
      }
      if (RS) {
        if (p.res_period) {
#pragma unroll
          for (int r = 0; r < R; ++r) src[r] %= p.res_period;
        }
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) src[r] /= p.rows_per_sample;
      }
      const float* base = (RS ? res : p.rowvec) + n;
      const int ld = RS ? p.ld_res : p.ld_rowvec;
#pragma unroll
      for (int r = 0; r < R; ++r) d[r] = *(const float4*)(base + (int64_t)src[r] * ld);
    };
    float4 g[2][R], gt[2][TB ? R : 1];
    issue(0, g[0], gt[0]);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b + 1 < NB) issue(b + 1, g[(b + 1) & 1], gt[(b + 1) & 1]);
      float4 v[R];
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = *(const float4*)(sC + ((b * R + r) * RPP + row0) * WNS + c0);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float4 t4 = UNI ? rv0 : g[b & 1][r];
        v[r].x = __builtin_fmaf(v[r].x, alpha, bias_v[0]) + t4.x;
        v[r].y = __builtin_fmaf(v[r].y, alpha, bias_v[1]) + t4.y;
        v[r].z = __builtin_fmaf(v[r].z, alpha, bias_v[2]) + t4.z;
        v[r].w = __builtin_fmaf(v[r].w, alpha, bias_v[3]) + t4.w;
        if constexpr (TB) {
          const float4 u4 = gt[b & 1][r];
          v[r].x += u4.x; v[r].y += u4.y; v[r].z += u4.z; v[r].w += u4.w;
        }
        // the value exists here, for every lane: the arithmetic (and with it the counted wait for the operand load) must not sink into the
        // predicated store below, where a lane-masked wait would be repeated, as vmcnt(0), in front of every later store
        asm volatile("" : "+v"(v[r].x), "+v"(v[r].y), "+v"(v[r].z), "+v"(v[r].w));
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int m = m_base + (b * R + r) * RPP + row0;
        if (FULL || m < m_end) *(float4*)(outf + (int64_t)m * p.ld_out + n) = v[r];
      }
    }
  };
  // (a partial slab's stores are predicated per lane; the waits the compiler counts across such a store assume it was not issued, so
  // they retire some stores too: the full slab, which is every slab but the last rows of a launch, gets straight-line code)
  const bool uni = RV && m_base / p.rows_per_sample == m_last / p.rows_per_sample;
  const bool full = m_base + WM <= m_end;
  if (RV && uni) {
    if (full) run(std::true_type{}, std::true_type{});
    else run(std::true_type{}, std::false_type{});
  } else {
    if (full) run(std::false_type{}, std::true_type{});
    else run(std::false_type{}, std::false_type{});
  }
}

// The slab of a wave is private to it and the LDS operations of one wave complete in order: between its slab writes and its row reads
// (and between the reads of one slab and the writes of the next) a wave needs its own LDS wait, not a workgroup barrier.
__device__ __forceinline__ void igemm_epilogue_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// sC: this wave's WM x WNS fp32 slab; (m_base, n_base): its position in the output; rows >= m_end are not stored; bz: batched-GEMM index.
// RMAX: the most passes per batch the calling kernel has registers for (no kernel may gain scratch); 0 = it keeps the serial loop.
// TBP: the kernel also has the registers for the pipelined row-table form (a second operand stream); else a table takes the serial loop.
template <int WM, int WNS, int RMAX = PD_EPI_R, bool TBP = true>
__device__ __forceinline__ void igemm_epilogue(const pd_igemm_args& p, const float* sC, int lane, int m_base, int m_end, int n_base, int bz) {
  float* outf = p.out_f32 ? p.out_f32 + (int64_t)bz * p.out_batch_stride : nullptr;
  pd_bf16* outb = p.out_bf16 ? p.out_bf16 + (int64_t)bz * p.outb_batch_stride : nullptr;
  pd_bf16* outbl = p.out_bf16_lo ? p.out_bf16_lo + (int64_t)bz * p.outb_batch_stride : nullptr;
  const float* res = p.residual ? p.residual + (int64_t)bz * p.res_batch_stride : nullptr;
  const bool rvp = p.rowvec != nullptr, mup = p.mul != nullptr, rsp = res != nullptr, ofp = outf != nullptr, obp = outb != nullptr,
             olp = outbl != nullptr;
  const int actv = (p.debug_flags & 4) ? 0 : p.act;
  const bool rtp = p.rowtab != nullptr;              // (only the residual-stream writers with a residual have a compiled form of their own for it)
  constexpr int GELU = PD_ACT_GELU;
  if (p.vec_epilogue == 2 && !rtp && !rvp && !mup && !rsp && !ofp && obp && !olp && (actv == 0 || actv == GELU)) {
    // bf16-only producers: QKV (no activation), FFN-1 (GELU)
    if (actv == 0) igemm_epilogue_rows<WM, WNS, 8, 0, 0, 0, 0, 0, 1, 0>(p, sC, lane, m_base, m_end, n_base, outf, outb, outbl, res);
    else igemm_epilogue_rows<WM, WNS, 8, GELU, 0, 0, 0, 0, 1, 0>(p, sC, lane, m_base, m_end, n_base, outf, outb, outbl, res);
  } else if (p.vec_epilogue && ofp && !obp && !mup && actv == 0 && (rsp != rvp) && (!rtp || rsp)) {
    // fp32 residual-stream writers: proj / FFN-2 / conv-2 (+residual), conv-1 (+timestep embedding)
    // (pipelined unless debug_flags bit 32 asks for the serial loop; a lane whose four columns cross N takes the scalar path of that loop)
    constexpr int NP = WM / (64 / (WNS / 4));
    constexpr int R = RMAX == 0 ? 1 : RMAX < NP ? RMAX : NP;
    const bool serial = RMAX == 0 || (p.debug_flags & 32) || n_base + (lane % (WNS / 4)) * 4 + 3 >= p.N;
    if (rsp && rtp) {
      if (serial || !TBP) igemm_epilogue_rows<WM, WNS, 4, -1, 2, 2, 2, 2, 2, 2>(p, sC, lane, m_base, m_end, n_base, outf, outb, outbl, res);
      else if (!(p.debug_flags & 2)) igemm_epilogue_rows_f32<WM, WNS, 0, 1, R, TBP>(p, sC, lane, m_base, m_end, n_base, outf, res);
    } else if (rsp) {
      if (serial) igemm_epilogue_rows<WM, WNS, 4, 0, 0, 0, 1, 1, 0, 0>(p, sC, lane, m_base, m_end, n_base, outf, outb, outbl, res);
      else if (!(p.debug_flags & 2)) igemm_epilogue_rows_f32<WM, WNS, 0, 1, R>(p, sC, lane, m_base, m_end, n_base, outf, res);
    } else {
      if (serial) igemm_epilogue_rows<WM, WNS, 4, 0, 1, 0, 0, 1, 0, 0>(p, sC, lane, m_base, m_end, n_base, outf, outb, outbl, res);
      else if (!(p.debug_flags & 2)) igemm_epilogue_rows_f32<WM, WNS, 1, 0, R>(p, sC, lane, m_base, m_end, n_base, outf, res);
    }
  } else if (p.vec_epilogue == 2) {
    igemm_epilogue_rows<WM, WNS, 8, -1, 2, 2, 2, 2, 2, 2>(p, sC, lane, m_base, m_end, n_base, outf, outb, outbl, res);
  } else {
    igemm_epilogue_rows<WM, WNS, 4, -1, 2, 2, 2, 2, 2, 2>(p, sC, lane, m_base, m_end, n_base, outf, outb, outbl, res);
  }
}
