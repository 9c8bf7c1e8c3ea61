/*
 * prediff_hip.h -- C ABI of libprediff_hip.so: hand-written HIP (gfx950 / CDNA4) kernels for the
 * PreDiff sampling hot path (Earthformer-UNet denoiser, KL-VAE, DDPM/DDIM step epilogue).
 *
 * The reference (gaozhihan/PreDiff) is pure Python/PyTorch and has no FFI: the boundary it offers is the
 * Python call convention of its nn.Modules.  Each entry point below replaces the ATen op
 * sequence of the cited reference function; the prediff_amd Python modules (same class names / ctor kwargs / state_dict
 * schema as the reference) are the only callers.  All pointers are caller-owned DEVICE pointers, layouts are
 * channels-last, no entry point allocates, every launch goes to the given stream and every function returns
 * 0 on success or a negative pd_status (the Python side raises).  Paths below are relative to
 * /root/reference/src/prediff/.
 */
#ifndef PREDIFF_HIP_H
#define PREDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pd_stream_t;   /* hipStream_t */
typedef uint16_t pd_bf16;    /* raw bfloat16 bits */

enum pd_status { PD_OK = 0, PD_ERR_ARG = -1, PD_ERR_UNSUPPORTED = -2, PD_ERR_LAUNCH = -3 };
enum pd_act { PD_ACT_NONE = 0, PD_ACT_GELU = 1, PD_ACT_SILU = 2, PD_ACT_LEAKY = 3, PD_ACT_RELU = 4 };
/* Type of the 16-bit MFMA operands a call reads and writes (`pd_bf16` pointers then carry IEEE half bits): bfloat16 (8-bit mantissa, the
 * throughput engine) or IEEE half (11-bit significand at the same MFMA rate: the TF32-class engine -- the reference runs fp32 with
 * float32_matmul_precision "high", scripts/prediff/sevirlr/prediff_sevirlr_v1.yaml:63).  Weights must be packed in the same type.
 * The hi/lo split (fp32-class) forms exist for bfloat16 only. */
enum pd_operand { PD_OPERAND_BF16 = 0, PD_OPERAND_F16 = 1 };

/* Per-call options of the entry points that read / write 16-bit operands or have an A/B switch: passed on every call, NULL = all
 * defaults (bfloat16, production settings).  Nothing in this library is process-global: two engines in one process (the two-lane mode
 * runs two, each from its own host thread) cannot see each other's settings.  All-zero = defaults. */
typedef struct pd_call_opts {
  int32_t operand;                  /* enum pd_operand */
  int32_t attn_block_table_ids;     /* pd_attn_block_fused_ex: != 0 = load the token table even when an affine form is given (A/B; bit-identical) */
  int32_t ffn_rows128;              /* pd_ffn_fused at units 256: != 0 = the 128-row kernel instead of ffn64_kernel (A/B) */
  int32_t groupnorm_two_launches;   /* pd_groupnorm_silu: != 0 = always the statistics + apply pair of launches (A/B) */
  int32_t pair_form;                /* pd_attn_ffn_pair at units 256: 1 / 2 = groups per wave with four waves (64- / 128-row tiles), 8 = eight
                                       waves of one group (128-row tiles), whatever the grid; 0 = automatic */
  int32_t ffn_debug_flags;          /* profiling ablations of the fused FFN (scripts/bench_ffn.py); 0 in production */
  int32_t attn_block_debug_flags;   /* profiling ablations of the fused attention block (scripts/bench_attn_block.py) */
  int32_t small_grid;               /* != 0: the caller allows kernel choices that depend on the launch size (the engine's small-batch mode; results
                                       then are not bit-identical across batch sizes).  pd_groupnorm_silu: finer channel chunks (twice the workgroups)
                                       at <= 1024 rows per sample when the default chunks would leave more than half of the CUs idle */
  int32_t w_fold;                   /* ABI 4.  pd_attn_ffn_pair / pd_attn_ffn_pair_split: != 0 = the weight stream holds W_hi AND W_lo chunks
                                       (packing.pack_pair_block(fold=True): twice the chunks; precision="fp16x2"), two MFMA products per k-step
                                       against the once-rounded activations.  One 16-slot group per wave only (pair_form 2 is refused) */
  int32_t reserved1;
  unsigned long long* trace;        /* device buffer for per-phase clock stamps of the fused kernels (pd_ffn_fused, pd_attn_block_fused_ex,
                                       pd_attn_ffn_pair in a -DPD_PAIR_TRACE=1 / -DPD_PAIR_DEBUG=1 build), or NULL (production) */
} pd_call_opts;
int pd_sizeof_call_opts(void);

int pd_abi_version(void);
const char* pd_last_error(void);
int pd_sizeof_igemm_args(void);         /* binding self-check: sizeof the argument structs below */
int pd_sizeof_cuboid_attn_args(void);

/* ---------------------------------------------------------------------------------------------------
 * pd_igemm: implicit-GEMM on the MFMA pipes (bf16 x bf16 -> fp32 accumulate).
 *   out[m, n] = act(alpha * sum_{tap, c} A[src(m, tap), c] * W[tap, n, c] + bias[n] + rowvec[m / rows_per_sample, n])
 *               (* mul[m, n]) (+ residual[m % res_period, n])
 * With taps == 1 it is nn.Linear (cuboid_transformer.py:849 qkv, :951 proj, :201-203 ffn_1/ffn_2, :294
 * reduction; cuboid_transformer_unet.py:492 final_proj; taming/attention.py:145-147,180).  With taps == 27 it
 * is nn.Conv3d 3x3x3 pad 1 on (B,T,H,W,C) (models/time_embed.py:92,119); with taps == 9 nn.Conv2d 3x3 incl. the
 * nearest x2 up-sampling fused in the gather (cuboid_transformer.py:373-375, taming/resnet.py:128-141) and the
 * stride-2 / pad (0,1,0,1) down-sampling (taming/resnet.py:183-188).  split != 0 runs the 3-product
 * bf16 hi/lo decomposition (fp32-class accuracy) on {A, A_lo} x {W, W_lo}.
 * ------------------------------------------------------------------------------------------------- */
typedef struct pd_igemm_args {
  const pd_bf16* A;        /* activations, channels-last rows of lda elements */
  const pd_bf16* A_lo;     /* split mode: low part (else NULL) */
  const pd_bf16* W;        /* weights packed [tap][N][ldw] (K contiguous) */
  const pd_bf16* W_lo;
  const float* bias;       /* [N] or NULL */
  const float* rowvec;     /* [n_samples][ld_rowvec] or NULL (timestep-embedding add) */
  const float* residual;   /* fp32 [*, ld_res] or NULL */
  const float* mul;        /* fp32 [M, ld_mul] or NULL (gated FFN) */
  float* out_f32;          /* [M, ld_out] or NULL */
  pd_bf16* out_bf16;       /* [M, ld_outb] or NULL */
  pd_bf16* out_bf16_lo;    /* split mode low part of the bf16 output or NULL */
  int64_t a_batch_stride, w_batch_stride, out_batch_stride, outb_batch_stride, res_batch_stride;  /* grid.z */
  int64_t w_tap_stride;    /* elements between taps of W */
  int32_t nbatch;
  int32_t M, N, Cin, taps; /* Cin: K per tap, multiple of 64 (zero padded) */
  int32_t lda, ldw;
  int32_t B, Ti, Hi, Wi, To, Ho, Wo;      /* conv geometry (input dims before up-sampling) */
  int32_t KT, KH, KW, st, sh, sw, pt, ph, pw, ut, uh, uw;
  int32_t vT, vH, vW;      /* size of the (virtually up-sampled) input the taps are bounds-checked against; 0 = Ti*ut etc. */
  int32_t rows_per_sample, ld_rowvec, ld_res, res_period, ld_mul, act, ld_out, ld_outb, split;
  float alpha;
  int32_t tile;            /* 0 = auto; 1 = 128x128, 2 = 64x64, 3-6 = pipeline variants of 128x128, 7 = 256x256 (8 waves, taps streamed), 8 / 9 = 128x64 / 64x128,
                              10 / 11 = 256x256 halo-staged Conv3d 3x3x3 (16 x 16 / 8 x 8 frames, one-product 16-bit operands; else as 7) */
  int32_t vec_epilogue;    /* set by the library */
  uint32_t a_bytes, w_bytes; /* set by the library: extent of one A / W batch (buffer-descriptor bounds) */
  int32_t debug_flags;     /* profiling ablations only: 1 skip main loop, 2 skip stores, 4 skip activation, 8 keep the dense tap loop of the 256 x 256 Conv3d kernels (tile 11 skips nothing: no effect),
                              16 the automatic choice keeps the tap-streamed 256 x 256 kernel where it would take a halo-staged one (tile 10 or 11), 64 four-phase K-tile (0 in production),
                              128 (tests of pd_igemm_mx, which alone reads it; pd_igemm ignores it) K-split into two to four slices whenever a workspace is given, whatever the
                              grid: the split form at shapes too short (fewer than 32 K-tiles) to split by themselves,
                              256 the halo-staged Conv3d kernels (tile 10 or 11) keep the MFMAs of the row tiles that read only the zero ring (the dense schedule; identical bits) */
  int32_t ksplit;          /* set by the library: K-slices of a split-K launch (1 = none) */
  float* splitk_ws;        /* caller workspace for split-K partial sums (fp32, splitk_ws_elems elements) or NULL: without it a launch
                              is never split.  Used for small grids (few trajectories per launch): the K loop of a long-K launch is cut
                              into slices that run as separate workgroups, then summed in slice order (deterministic) with the epilogue */
  int64_t splitk_ws_elems;
  int32_t fp8;             /* != 0: A and W hold OCP e4m3 bytes (lda / ldw / strides count elements = bytes; Cin % 128 == 0, lda/ldw % 16 == 0);
                              the tensor scales go in alpha.  Long-K row-wise linear and stride-1 convolution launches only (the 256 x 256
                              kernel, v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales); no hi/lo `split`, no batch.  With a
                              `splitk_ws` small grids still take the split-K route (fp32 slabs), unless the OUTPUT is e4m3 (below) */
  int32_t out_fp8_log2;    /* k > 0: out_bf16 points to OCP e4m3 BYTES (ld_outb counts bytes) and receives e4m3(v * 2^k), round to nearest
                              even, saturating at +-448 -- the A operand of a following fp8 launch (8-column vector epilogue: N % 8 == 0,
                              no out_bf16_lo; such a launch is never K-split, with or without `splitk_ws`).  0: bf16 output */
  int32_t operand;         /* enum pd_operand: type of A, W and out_bf16 (no `split`, no `fp8` with PD_OPERAND_F16) */
  int32_t disable_256;     /* A/B: != 0 = never hand this launch to the 256 x 256 kernel */
  int32_t min_k_256;       /* A/B: smallest K (taps * Cin) of a launch the automatic choice gives to the 256 x 256 kernel; 0 = default (1024) */
  int32_t splitk_max_tiles;/* A/B: split-K only for grids of at most this many 256 x 256 tiles; 0 = default (128), < 0 = never split */
  int32_t w_fold;          /* ABI 4.  f > 0: TWO weight products per filter tap (precision="fp16x2": W = W_hi + W_lo in the 16-bit operand type,
                              the activations rounded once) -- `taps` = 2 f, W holds the f taps of W_hi followed by the f taps of W_lo, and the
                              K loop walks the activation gather of tap (t mod f) against weight slab t: D = A W_hi^T + A W_lo^T in one fp32
                              accumulator.  f = KT * KH * KW (1 for a row-wise linear layer).  0: one product (taps = KT * KH * KW) */
  int32_t rowtab_rows;     /* rows of `rowtab` (> 0 with a table; was reserved0) */
  const float* rowtab;     /* (appended; pd_sizeof_igemm_args grows by 8)  fp32 [rowtab_rows][N] or NULL: out row m += rowtab[m % rowtab_rows], added LAST -- after alpha, bias,
                              row vector, activation, gate and residual, i.e. ((acc + bias) + residual) + table: the bits of a
                              pd_add_rowtable launch behind this one (the positional table behind first_proj's second convolution).
                              fp32 output only, never together with a split-K workspace */
} pd_igemm_args;
int pd_igemm(const pd_igemm_args* a, pd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * MX (OCP microscaling) e4m3 operands: every 32 consecutive K elements of a row share one E8M0 scale byte (DESIGN.md section 7
 * states the format).  An MX operand is two byte arrays: the payload, rows of `ld` bytes, and the scales, rows of `ld / 32`
 * bytes; columns [K, ld) are padding (zero payload, scale byte 0).  pd_igemm_mx reads operands with ld % 128 == 0, so that a
 * 128-element K-tile never leaves a row (for a convolution: never spans two filter taps).
 * ------------------------------------------------------------------------------------------------- */
typedef struct pd_mx_operands {
  const uint8_t* a_scales;    /* [input rows][ld_a_scales] E8M0 bytes of A (input rows: B * Ti * Hi * Wi, as the rows of A) */
  const uint8_t* w_scales;    /* [tap][N][ld_w_scales] E8M0 bytes of W */
  int64_t w_scale_tap_stride; /* bytes between the taps of w_scales */
  int32_t ld_a_scales, ld_w_scales;   /* = lda / 32, ldw / 32 (multiples of 4) */
  int32_t reserved0, reserved1;
} pd_mx_operands;
int pd_sizeof_mx_operands(void);

/* pd_igemm on MX operands: A and W hold e4m3 payload bytes (lda / ldw / strides count bytes; Cin = the padded K per tap, Cin % 128 == 0,
 * lda, ldw % 128 == 0), `mx` their block scales; the scaled MFMA applies both scale bytes of every 32-element block.  Everything else
 * (geometry, epilogue, alpha, split-K through `splitk_ws`) as pd_igemm with fp8 != 0; `fp8`, `split`, `w_fold`, `operand`, `tile` and
 * `out_fp8_log2` of `a` must be 0 (the library sets what it needs).  Row-wise linear layers and stride-1, un-upsampled convolutions. */
int pd_igemm_mx(const pd_igemm_args* a, const pd_mx_operands* mx, pd_stream_t stream);

/* fp32 rows -> MX e4m3: q (rows, ld) payload bytes, scales (rows, ld / 32); x rows of ld_x floats; K % 32 == 0, ld % 32 == 0, ld >= K.
 * Per block: scale byte = clamp(127 + e, 0, 254) with e = floor(log2(amax)) - 8, one more where amax * 2^-e would exceed 448 (so that
 * no payload saturates); payload = e4m3(x * 2^-e), round to nearest even.  An all-zero block: scale byte 0, zero payload.  Non-finite
 * input is the caller's error. */
int pd_quantize_mx(const float* x, uint8_t* q, uint8_t* scales, int64_t rows, int K, int ld_x, int ld, pd_stream_t stream);

/* pd_layernorm with an MX output (the A operand of a pd_igemm_mx linear): out (rows, ld_out) payload, scales (rows, ld_out / 32);
 * C % 32 == 0, ld_out % 32 == 0, C <= ld_out <= the last 256-column block of C. */
int pd_layernorm_mx(const float* x, const float* gamma, const float* beta, uint8_t* out, uint8_t* scales, int64_t rows, int C, int ld_out,
                    float eps, pd_stream_t stream);

/* pd_groupnorm_silu with an MX output (the A operand of a pd_igemm_mx convolution): out (B * S, ld_out) payload, scales
 * (B * S, ld_out / 32).  C % 32 == 0, C/4 divides 256, 4 | C/G, ld_out % 32 == 0, ld_out >= C, ld_out - C < 128 (pad columns are
 * written: zero payload, scale byte 0). */
int pd_groupnorm_silu_mx(const float* x, const float* gamma, const float* beta, const float* ss_scale, const float* ss_shift, int ld_ss,
                         double* partials, uint8_t* out, uint8_t* scales, int B, int S, int C, int G, int ld_out, float eps, int silu,
                         pd_stream_t stream);

/* nn.LayerNorm(eps, affine) over the last dim C of fp32 rows -> bf16 (hi[, lo]) rows of ld_out elements
 * (pad columns [C, ld_out) are written as zero).  cuboid_transformer.py:813 (attn pre-norm), :197 (FFN pre-norm). */
int pd_layernorm(const float* x, const float* gamma, const float* beta, pd_bf16* out, pd_bf16* out_lo,
                 int64_t rows, int C, int ld_out, float eps, const pd_call_opts* opts, pd_stream_t stream);

/* pd_layernorm with an OCP e4m3 output (the A operand of an fp8 pd_igemm launch): out[row, c] = e4m3(y * fp8_scale), round to nearest
 * even, saturating at +-448; rows of ld_out bytes (pad columns zero). */
int pd_layernorm_fp8(const float* x, const float* gamma, const float* beta, uint8_t* out, int64_t rows, int C, int ld_out, float eps,
                     float fp8_scale, pd_stream_t stream);

/* PatchMerging3D gather + LayerNorm(prod(ds)*C): x (B,T,H,W,C) fp32 -> (B,T/dt,H/dh,W/dw, dt*dh*dw*C) bf16, zero padding at
 * the far edge.  cuboid_transformer.py:274-293. */
int pd_patch_merge_layernorm(const float* x, const float* gamma, const float* beta, pd_bf16* out, pd_bf16* out_lo,
                             int B, int T, int H, int W, int C, int dt, int dh, int dw, int ld_out, float eps,
                             pd_stream_t stream);
/* The same with per-call options and the padding rule of the gather: pad_nearest != 0 = PatchMerging3D(padding_type="nearest") on a shape the down-sampling
 * does not divide (models/utils.py:228-256: the padded grid is the nearest-neighbour resize of the tensor); 0 = zero padding. */
int pd_patch_merge_layernorm_ex(const float* x, const float* gamma, const float* beta, pd_bf16* out, pd_bf16* out_lo,
                             int B, int T, int H, int W, int C, int dt, int dh, int dw, int ld_out, float eps, int pad_nearest,
                             const pd_call_opts* opts, pd_stream_t stream);

/* nn.GroupNorm(G, C, eps) [+ optional (1+scale)*y+shift] [+ SiLU] over channels-last x (B, S, C) fp32 -> bf16 rows of
 * ld_out elements.  `partials` is caller workspace of B*nchunk*G*2 doubles (nchunk from pd_groupnorm_nchunk).
 * models/time_embed.py:89-93,115-120,155-166; taming/resnet.py:457-458,478-485; taming/vae.py:82-84. */
int pd_groupnorm_nchunk(int S, int C);
int pd_groupnorm_silu(const float* x, const float* gamma, const float* beta, const float* ss_scale,
                      const float* ss_shift, int ld_ss, double* partials, pd_bf16* out, pd_bf16* out_lo,
                      int B, int S, int C, int G, int ld_out, float eps, int silu, const pd_call_opts* opts, pd_stream_t stream);

/* The statistics pass of pd_groupnorm_silu alone: stats[b][g] = {mean, rstd} (fp32) of nn.GroupNorm(G, C, eps) over channels-last
 * x (B, S, C); partials as for pd_groupnorm_silu.  For consumers that normalise on the fly (pd_conv2d_gn_silu). */
int pd_groupnorm_stats(const float* x, double* partials, float* stats, int B, int S, int C, int G, float eps, pd_stream_t stream);

/* ResnetBlock2D's  GroupNorm -> SiLU -> Conv2d 3x3 (stride 1, zero padding 1) [+ bias] [+ fp32 residual]  in one launch
 * (taming/resnet.py:454-495 at temb = None): x (N, H, W, Cin) fp32 channels last is normalised with stats (N, G, 2) = {mean, rstd}
 * from pd_groupnorm_stats, passed through SiLU and rounded to bf16 inside the kernel's LDS halo tile; W packed bf16 [9][Cout][Cin]
 * (prediff_amd/packing.py:pack_conv, taps (ky, kx)); out (N, H, W, Cout) fp32, may alias residual.  Supported when
 * pd_conv2d_gn_silu_supported(H, W, Cin, Cout, G): H % 8 == 0, W % 16 == 0, Cin % 64 == 0, Cout % 128 == 0, (Cin / G) % 4 == 0;
 * otherwise use pd_groupnorm_silu + pd_igemm. */
int pd_conv2d_gn_silu_supported(int H, int W, int Cin, int Cout, int G);
int pd_conv2d_gn_silu(const float* x, const float* stats, const float* gamma, const float* beta, const pd_bf16* W, const float* bias,
                      const float* residual, float* out, int N, int H, int W_, int Cin, int Cout, int G, const pd_call_opts* opts,
                      pd_stream_t stream);

/* The VAE's Upsample2D (taming/resnet.py:128-141): nearest x2 up-sampling -> Conv2d 3x3 (stride 1, zero padding 1) [+ bias] in one launch of the
 * same tile kernel: x (N, H / 2, Wd / 2, Cin) fp32 channels last -> out (N, H, Wd, Cout) fp32; H, Wd are the OUTPUT size.  The halo of a pixel
 * tile is staged from the half-resolution source (no normalisation in front of this convolution): no 16-bit cast pass over the input, no gather
 * per filter tap.  Geometry as pd_conv2d_gn_silu_supported(H, Wd, Cin, Cout, 1). */
int pd_conv2d_up2(const float* x, const pd_bf16* W, const float* bias, float* out, int N, int H, int Wd, int Cin, int Cout,
                  const pd_call_opts* opts, pd_stream_t stream);

/* pd_groupnorm_silu with an OCP e4m3 output (the A operand of an fp8 pd_igemm launch): out[b, s, c] = e4m3(y * fp8_scale),
 * round to nearest even, saturating at +-448; rows of C bytes.  C % 4 == 0, C/4 divides 256, 4 | C/G. */
int pd_groupnorm_silu_fp8(const float* x, const float* gamma, const float* beta, const float* ss_scale,
                          const float* ss_shift, int ld_ss, double* partials, uint8_t* out, int B, int S, int C, int G,
                          float eps, int silu, float fp8_scale, pd_stream_t stream);

/* Data gradient of pd_groupnorm_silu on contiguous channels-last rows (ld = C): dx (B, S, C) from x, dy and the forward's
 * partial sums (mean / rstd are re-derived from them); bwd_partials: B * pd_groupnorm_nchunk(S, C) * G * 2 doubles of scratch.
 * gamma / beta get no gradient (frozen guidance network).  C must divide 256.  What autograd derives for
 * models/time_embed.py:89-120,134-169 (GroupNorm32 -> SiLU) inside the knowledge-alignment gradient (alignment.py:60-66). */
int pd_groupnorm_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta,
                          const double* fwd_partials, double* bwd_partials, float* dx, int B, int S, int C, int G,
                          float eps, int silu, pd_stream_t stream);

/* fp32 rows -> bf16 (hi[, lo]) rows with optional row gather (rows_per_sample_out rows taken from offset row_off inside
 * each rows_per_sample_in block) and zero padded columns.  Used for un-normalised GEMM inputs
 * (cuboid_transformer_unet.py:492 x[:, in_len:], time_embed.py:169 skip_connection input, cuboid_transformer.py:373). */
int pd_cast_rows(const float* x, pd_bf16* out, pd_bf16* out_lo, int64_t n_samples, int rows_per_sample_in, int row_off,
                 int rows_per_sample_out, int C, int ld_in, int ld_out, const pd_call_opts* opts, pd_stream_t stream);

/* Cuboid self-attention core: softmax(scale * q k^T + rel_pos_bias [masked]) v per (sample, cuboid, head).
 * qkv: (B, ntok, 3*C) rows [q | k | v], head h at columns h*hd; tok_index[(nc, vol)] = flat token id or -1 for a padded
 * slot (zero q/k/v that still takes softmax mass); bias (heads, vol, vol) fp32; mask (nc, vol, vol) u8 or NULL.
 * Output o: (B, ntok, C) bf16 (and/or fp32) in natural token order.  MFMA path (vol <= 16, bf16 qkv) or generic fp32 path.
 * cuboid_transformer.py:839-861,947-949,956-962 + 388-467 (reorder) + 470-560 (mask, masked_softmax). */
typedef struct pd_cuboid_attn_args {
  const pd_bf16* qkv_bf16;   /* one of qkv_bf16 / qkv_f32 */
  const float* qkv_f32;
  const int32_t* tok_index;
  const float* bias;
  const uint8_t* mask;
  pd_bf16* out_bf16;
  pd_bf16* out_bf16_lo;
  float* out_f32;
  int32_t B, ntok, C, heads, nc, vol, ld_qkv, ld_out;
  float scale;
  int32_t force_generic;
  int32_t out_fp8_log2;      /* k > 0 (MFMA cores, cuboid volume <= 64 only): out_bf16 points to e4m3 BYTES (ld_out counts bytes) and receives
                                e4m3(o * 2^k), round to nearest even, saturating: the A operand of an fp8 proj launch.  0: bf16 output */
  const int32_t* tok_out;    /* NULL: a slot's result goes to the token it was gathered from (tok_index).  Else [nc][vol]: the token that
                                RECEIVES the slot's result, -1 = nobody -- padding_type "nearest" on a non-divisible shape, where the padded grid
                                is a nearest-neighbour resize of the tokens (several slots read one token) and the un-padding resizes back
                                (models/utils.py:228-270).  Runs on the generic core. */
  int32_t operand;           /* enum pd_operand: type of qkv_bf16 / out_bf16 (MFMA cores; the generic core reads either) */
  int32_t qkv_fp8_log2;      /* k > 0 (ABI 4; MFMA core, cuboid volume <= 64, head_dim % 32 == 0): qkv_bf16 points to OCP e4m3 BYTES holding
                                q, k, v * 2^k (ld_qkv counts bytes) -- what an fp8 pd_igemm launch writes with out_fp8_log2 = k; q k^T and attn v
                                then run on the fp8 MFMA (probabilities as e4m3(P * 256)), fp32 scores / softmax / accumulation
                                (BASELINE.json configs[4]; cuboid_transformer.py:849-861,947-952).  0: 16-bit / fp32 q, k, v */
} pd_cuboid_attn_args;
int pd_cuboid_attention(const pd_cuboid_attn_args* a, pd_stream_t stream);

/* Data gradient of pd_cuboid_attention (fp32): given qkv (B, ntok, 3C) and d_out (B, ntok, C), both in natural token order, writes
 * d_qkv (B, ntok, 3C).  The probabilities are recomputed from qkv + bias; bias table and weights get no gradient (sampling-time
 * guidance only).  Replaces what torch.autograd derives for cuboid_transformer.py:852-861,947-949 when the knowledge-alignment
 * gradient is taken (prediff/knowledge_alignment/alignment.py:60-66 through models.py:459-528).  vol <= 64, head_dim <= 128. */
int pd_cuboid_attention_bwd(const float* qkv, const float* d_out, const int32_t* tok_index, const float* bias,
                            const uint8_t* mask, float* d_qkv, int B, int ntok, int C, int heads, int nc, int vol,
                            int ld_qkv, int ld_dout, int ld_dqkv, float scale, pd_stream_t stream);

/* Row softmax of fp32 scores (rows, n) -> bf16 probabilities (taming/attention.py:176, computed in fp32). */
int pd_softmax_rows(const float* x, pd_bf16* out, pd_bf16* out_lo, int64_t rows, int n, int ld_in, int ld_out,
                    const pd_call_opts* opts, pd_stream_t stream);

/* Denoiser stem: cat([cond, x], T) + observation-indicator channel -> fp32 (B, T_in+T_out, H, W, C+1) rows of ld_out
 * elements.  cuboid_transformer_unet.py:425-428. */
int pd_unet_build_input(const float* x, const float* cond, float* out, int B, int T_in, int T_out, int HW, int C,
                        int ld_out, pd_stream_t stream);

/* pd_unet_build_input that also writes the bfloat16 copy of its rows (out16: rows of ld16 elements, zero padded: what pd_cast_rows
 * makes of `out`), in the same pass: the A operand of the stem's skip convolution.  C a multiple of 4, ld16 a multiple of 4 in
 * (C, 2 C]; x / cond 16 B aligned.  bfloat16 only. */
int pd_unet_build_input16(const float* x, const float* cond, float* out, pd_bf16* out16, int B, int T_in, int T_out, int HW,
                          int C, int ld_out, int ld16, pd_stream_t stream);

/* Sinusoidal timestep embedding [cos(t f_k) | sin(t f_k)] (models/utils.py:68-88), t int64 (B,) -> fp32 (B, dim).
 * freqs: dim/2 fp32 frequencies exp(-ln(max_period) k / half), computed once on the host exactly as the reference does. */
int pd_timestep_embedding(const int64_t* t, const float* freqs, float* out, int B, int dim, pd_stream_t stream);

/* Small dense layer (one row per workgroup column, M <= 65535 rows): out = act_out(W act_in(x) + b), fp32 throughout (TimeEmbedLayer models/time_embed.py:15-24,
 * emb_layers :105-113).  W (N, K) row-major fp32. */
int pd_linear_small(const float* x, const float* W, const float* b, float* out, int M, int K, int N, int act_in,
                    int act_out, pd_stream_t stream);

/* The whole timestep-embedding chain of the denoiser (pd_timestep_embedding -> pd_linear_small (SiLU out) -> pd_linear_small -> one
 * SiLU-in pd_linear_small per TimeEmbedResBlock) in four launches: sinusoid, first layer, second layer, all `nproj` projections.
 * Every buffer the chain writes is written (sin_out (B, dim), h1 (B, E), temb (B, E), proj_out[q] (B, proj_N[q])), bit-equal to the
 * chain's: per output the summation order is pd_linear_small's.  A wave keeps one weight row in registers for all B rows and the
 * activation rows are staged in LDS once per eight columns, so a weight is read once per launch, not once per row.  (One launch would need a device-wide wait between the layers -- each output of
 * a layer reads every output of the one before -- which this library does not do.)  dim: a multiple of 4 up to 256; E: one up to
 * 1024 (pd_time_embed_supported); W0 (E, dim), W2 (E, E), proj_W[q] (proj_N[q], E) row-major fp32, 16 B aligned; the bias pointers
 * may be NULL.  proj_* are HOST arrays of nproj <= PD_TIME_EMBED_MAX_PROJ entries. */
#define PD_TIME_EMBED_MAX_PROJ 8
int pd_time_embed_supported(int dim, int E);
int pd_time_embed(const int64_t* t, const float* freqs, const float* W0, const float* b0, const float* W2, const float* b2,
                  const float* const* proj_W, const float* const* proj_b, float* const* proj_out, const int* proj_N, int nproj,
                  float* sin_out, float* h1, float* temb, int B, int dim, int E, pd_stream_t stream);

/* x[b, s, c] += table[s, c] (PosEmbed with the three tables pre-summed; cuboid_transformer.py:65-90) */
int pd_add_rowtable(float* x, const float* table, int64_t n_samples, int rows_per_sample, int C, pd_stream_t stream);

/* out = a + b (U-Net skip add, cuboid_transformer_unet.py:473-474) */
int pd_add(const float* a, const float* b, float* out, int64_t n, pd_stream_t stream);

/* DDPM ancestral step from the predicted noise (latent_diffusion.py:553-566,592-596,620-631):
 *   z0 = c_recip[t] z - c_recipm1[t] eps ; mean = c1[t] z0 + c2[t] z [- exp(.5 logvar[t]) shift] ;
 *   out = mean + (t != 0) exp(.5 logvar[t]) temperature noise.   coef: 5 fp32 tables of length T:
 *   [sqrt_recip_ac | sqrt_recipm1_ac | post_mean_coef1 | post_mean_coef2 | post_logvar_clipped]. */
int pd_ddpm_step(const float* zt, const float* eps, const float* noise, const float* mean_shift, const int64_t* t,
                 const float* coef, int T, float* out, int B, int64_t per_sample, float temperature, int clip_denoised,
                 pd_stream_t stream);

/* DDIM step (no reference implementation; stable-diffusion lineage of diffusion/utils.py:42-70):
 *   z0 = (z - sqrt(1-a_t) eps)/sqrt(a_t) ; out = sqrt(a_prev) z0 + sqrt(1-a_prev-sigma^2) eps + sigma noise.
 *   coef (B,3) fp32 per sample: [a_t, a_prev, sigma]. */
int pd_ddim_step(const float* zt, const float* eps, const float* noise, const float* coef, float* out, int B,
                 int64_t per_sample, pd_stream_t stream);

/* Knowledge-alignment guided DDIM step: out = <pd_ddim_step> - gamma * shift, the subtraction last, so a zero shift
 *   gives pd_ddim_step's result bit for bit.  coef4 (B,4) fp32 per sample: [a_t, a_prev, sigma, gamma]; shift: fp32 like zt. */
int pd_ddim_step_guided(const float* zt, const float* eps, const float* noise, const float* shift, const float* coef4, float* out, int B, int64_t per_sample, pd_stream_t stream);

/* DPM-Solver++(2M) step, data prediction (no reference implementation): per sample, with the row [a_t, c_x, c_d, w] of
 *   coef4 (B,4) fp32 (schedule.make_dpmpp_2m_coefficients),
 *   x0 = (z - sqrt(1-a_t) eps)/sqrt(a_t) ; D = w != 0 ? x0 + w (x0 - hist) : x0 ; out = c_x z + c_d D ; hist <- x0.
 *   hist: fp32 like zt, the previous step's x0, updated in place; it is not read where w == 0 (first step: it may hold anything, NaN included).
 *   out must not alias zt, eps or hist. */
int pd_dpmpp_2m_step(const float* zt, const float* eps, float* hist, const float* coef4, float* out, int B, int64_t per_sample,
                     pd_stream_t stream);

/* Knowledge-alignment guided form: out = <pd_dpmpp_2m_step> - gamma * shift, the subtraction last, so a zero shift gives pd_dpmpp_2m_step's
 *   result bit for bit.  coef5 (B,5) fp32 per sample: [a_t, c_x, c_d, w, gamma]; shift: fp32 like zt. */
int pd_dpmpp_2m_step_guided(const float* zt, const float* eps, float* hist, const float* shift, const float* coef5, float* out, int B,
                            int64_t per_sample, pd_stream_t stream);

/* SDE-DPM-Solver++(2M) step (no reference implementation): pd_dpmpp_2m_step with a noise term.  Per sample, with the row
 *   [a_t, c_x, c_d, w, c_n] of coef5 (B,5) fp32 (schedule.make_dpmpp_2m_sde_coefficients),
 *   x0 and D as pd_dpmpp_2m_step ; out = c_x z + c_d D + c_n noise ; hist <- x0.
 *   noise: fp32 like zt, unit normal draws; it is not read where c_n == 0 (eta = 0: it may hold anything, NaN included), and the result
 *   there is pd_dpmpp_2m_step's bit for bit.  hist as in pd_dpmpp_2m_step.  out must not alias zt, eps, noise or hist. */
int pd_dpmpp_2m_sde_step(const float* zt, const float* eps, const float* noise, float* hist, const float* coef5, float* out, int B,
                         int64_t per_sample, pd_stream_t stream);

/* Knowledge-alignment guided form: out = <pd_dpmpp_2m_sde_step> - gamma * shift, the subtraction last, so a zero shift gives
 *   pd_dpmpp_2m_sde_step's result bit for bit.  coef6 (B,6) fp32 per sample: [a_t, c_x, c_d, w, c_n, gamma]; shift: fp32 like zt. */
int pd_dpmpp_2m_sde_step_guided(const float* zt, const float* eps, const float* noise, float* hist, const float* shift, const float* coef6,
                                float* out, int B, int64_t per_sample, pd_stream_t stream);

/* Held-region (inpainting) forms of the three step kernels ("Held regions"): the step and the hold in one launch.
 *   v    = the un-held kernel's result, the same operations in the same order (shift == NULL: un-guided, gamma is not read)
 *   held = k_n != 0 ? k_x hold_x0 + k_n hold_noise : k_x hold_x0
 *   out  = m == 0 ? v : m == 1 ? held : m held + (1 - m) v          with m = hold_mask, fp32 in [0, 1], 1 = held
 *   The two end points are selects: where m == 0 the output is the un-held kernel's bit for bit whatever hold_x0 / hold_noise hold
 *   (NaN included), where m == 1 nothing of v reaches it, and with the row (k_x, k_n) = (1, 0) it is hold_x0 bit for bit there.
 *   hold_x0 / hold_mask / hold_noise: fp32 like zt.  k_n is per sample: hold_noise is not read where k_n == 0 (it may hold anything),
 *   but the pointer must not be NULL.  hist is read and written as in the un-held kernels.  out must not alias an input.
 *   Coefficient rows, fp32 per sample (the un-held row, gamma, then k_x = sqrt(u), k_n = sqrt(1 - u); schedule.make_hold_coefficients):
 *     pd_ddim_step_held          coef6 (B,6): [a_t, a_prev, sigma, gamma, k_x, k_n]      noise may be NULL (eta = 0), as pd_ddim_step
 *     pd_dpmpp_2m_step_held      coef7 (B,7): [a_t, c_x, c_d, w, gamma, k_x, k_n]
 *     pd_dpmpp_2m_sde_step_held  coef8 (B,8): [a_t, c_x, c_d, w, c_n, gamma, k_x, k_n]   noise is not read where c_n == 0 */
int pd_ddim_step_held(const float* zt, const float* eps, const float* noise, const float* shift, const float* hold_x0, const float* hold_mask,
                      const float* hold_noise, const float* coef6, float* out, int B, int64_t per_sample, pd_stream_t stream);
int pd_dpmpp_2m_step_held(const float* zt, const float* eps, float* hist, const float* shift, const float* hold_x0, const float* hold_mask,
                          const float* hold_noise, const float* coef7, float* out, int B, int64_t per_sample, pd_stream_t stream);
int pd_dpmpp_2m_sde_step_held(const float* zt, const float* eps, const float* noise, float* hist, const float* shift, const float* hold_x0,
                              const float* hold_mask, const float* hold_noise, const float* coef8, float* out, int B, int64_t per_sample,
                              pd_stream_t stream);

/* The start rule of a held run: out = <the select above> with v = z and the rows coef2 (B,2) = [k_x, k_n] = [sqrt(a_0), sqrt(1 - a_0)].
 *   out may alias z, and noise may be z itself (the starting latent is the noise of the held part). */
int pd_hold_blend(const float* z, const float* x0, const float* mask, const float* noise, const float* coef2, float* out, int B,
                  int64_t per_sample, pd_stream_t stream);

/* Tiled sampling on a canvas larger than the model's window (prediff_amd/tiled.py).  Channels-last fp32 throughout.
 *   canvas (B, T, Hc, Wc, C); windows (B, nwin, T, h, w, C), batch-major; origin_yx (nwin, 2) int32 ON THE DEVICE, the (y, x) of each
 *   window's first cell, 0 <= y <= Hc - h and 0 <= x <= Wc - w (the library cannot read the table: the caller checks it.  A window
 *   whose origin is out of range is gathered as zeros and reads nothing; the blend never reads outside a window).
 * pd_window_gather: windows[b, k] = canvas[b, :, y_k : y_k + h, x_k : x_k + w, :].
 * pd_window_blend : canvas(cell) = sum over the windows k covering the cell, in ascending k, of weights[k, cell - origin_k] * windows[b, k,
 *   cell - origin_k], accumulated with fmaf from 0 in fp32 by the one thread that owns the canvas element: no atomics, so two launches
 *   agree bit for bit.  weights (nwin, h, w) fp32 arrive normalised (they sum to 1 over the windows that cover a cell); nothing is
 *   divided on the device.  Every canvas element is written; a cell no window covers becomes 0.
 * float4 access over C when C % 4 == 0 and both buffers are 16-byte aligned, scalar access otherwise. */
int pd_window_gather(const float* canvas, float* windows, const int32_t* origin_yx, int B, int nwin, int T, int Hc, int Wc, int h, int w,
                     int C, pd_stream_t stream);
int pd_window_blend(const float* windows, const float* weights, const int32_t* origin_yx, float* canvas, int B, int nwin, int T, int Hc,
                    int Wc, int h, int w, int C, pd_stream_t stream);

/* Rolling forecasts beyond the model's horizon (DESIGN.md §7 "Rolling forecasts"; prediff_amd/rollout.py): the context advance between
 *   two sampler runs, and the append of the kept frames, in one launch.  Channels-last fp32 throughout.
 *   ctx, ctx_next: window stacks (B, nwin, T_in, h, w, C); z: the forecast latent canvas (B, T_out, Hc, Wc, C); origin_yx as above (a
 *   window whose origin is out of range reads nothing from z and gets zeros for its new frames).  The plain module is nwin = 1,
 *   (h, w) = (Hc, Wc), origin (0, 0).  1 <= stride <= T_out.
 * With cat = [ctx ; z_scale * z] along T, ctx_next = cat[stride : stride + T_in] per window:
 *   ctx_next[b, k, i] = ctx[b, k, i + stride]                                              where i + stride < T_in,
 *   ctx_next[b, k, i] = z_scale * z[b, i + stride - T_in, y_k : y_k + h, x_k : x_k + w]    otherwise: ONE fp32 multiply per element
 *   (z_scale = float32(1 / scale_factor), rounded by the caller; 1.0f makes it a copy).
 * forecast (B, f_T, Hc, Wc, C), or NULL with f_cnt = 0: forecast[b, f_off + i] = z[b, i] for i < f_cnt <= T_out, unscaled, bit for bit;
 *   f_off + f_cnt <= f_T.  Every element of ctx_next and of those f_cnt frames is written exactly once by one thread (no atomics); no
 *   other element of either buffer is touched.  ctx_next and forecast must not overlap ctx, z or each other.  No synchronisation and
 *   no host reads: the launch can be captured.
 * float4 access over C when C % 4 == 0 and all five buffers are 16-byte aligned, scalar access otherwise; 64-bit element offsets. */
int pd_context_advance(const float* ctx, const float* z, const int32_t* origin_yx, float* ctx_next, float* forecast, int B, int nwin,
                       int T_in, int T_out, int Hc, int Wc, int h, int w, int C, int stride, float z_scale, int f_T, int f_off, int f_cnt,
                       pd_stream_t stream);

/* Layout glue for the frame-wise VAE: fp32 NCHW <-> channels-last NHWC (taming/autoencoder_kl.py:80-113 callers,
 * latent_diffusion.py:361-380,423-432). */
int pd_nchw_to_nhwc(const float* x, float* out, int N, int C, int HW, int ld_out, pd_stream_t stream);
int pd_nhwc_to_nchw(const float* x, float* out, int N, int C, int HW, int ld_in, pd_stream_t stream);

/* PositionwiseFFN.forward, pre-norm (cuboid_transformer.py:182-208) fused into one launch: out = x + W2 act(W1 LN(x) + b1) + b2.
 * x/out fp32 (M, C) (may alias), W1 bf16 (Hd, C), W2 bf16 (C, Hd) as packed for pd_igemm.  The hidden activations stay in LDS.
 * Supported when pd_ffn_fused_supported(C, Hd) (C in {64,128,256}, Hd % 64 == 0); otherwise use pd_layernorm + 2 x pd_igemm. */
int pd_ffn_fused_supported(int C, int Hd);
int pd_ffn_fused(const float* x, float* out, const float* gamma, const float* beta, const pd_bf16* W1, const float* b1,
                 const pd_bf16* W2, const float* b2, int64_t M, int C, int Hd, int act, float eps, const pd_call_opts* opts,
                 pd_stream_t stream);

/* Fused cuboid self-attention block, bf16 engine:  out = x + proj(attention(qkv(LayerNorm(x))))  for head_dim 64 and cuboid volume
 * <= 64 (CuboidSelfAttentionLayer.forward cuboid_transformer.py:812-966 + the residual of :1151), in place allowed (out == x).
 * x/out (B, ntok, C) fp32; Wqkv (3C, C) and Wp (C, C) bf16 row-major; bqkv (3C) / bp (C) fp32 or NULL; tok_index, bias, mask
 * as for pd_cuboid_attention.  Supported when pd_attn_block_fused_supported(C, heads, vol); otherwise use
 * pd_layernorm + pd_igemm + pd_cuboid_attention + pd_igemm. */
int pd_attn_block_fused_supported(int C, int heads, int vol);
int pd_attn_block_fused(const float* x, float* out, const float* gamma, const float* beta, const pd_bf16* Wqkv, const float* bqkv,
                        const pd_bf16* Wp, const float* bp, const int32_t* tok_index, const float* bias, const uint8_t* mask,
                        int B, int ntok, int C, int heads, int nc, int vol, float scale, float eps, pd_stream_t stream);
/* The same with a host-side hint: tok_affine = {n_inner, outer, inner, slot} (HOST pointer, or NULL) states that
 * tok_index[c][s] == (c / n_inner) * outer + (c % n_inner) * inner + s * slot for every cuboid c and slot s < vol (un-shifted, un-padded
 * axial cuboids; n_inner <= 0 = no such form): the kernel then computes the token ids instead of loading the table in front of
 * its row gather (bit-identical results either way). */
int pd_attn_block_fused_ex(const float* x, float* out, const float* gamma, const float* beta, const pd_bf16* Wqkv, const float* bqkv,
                           const pd_bf16* Wp, const float* bp, const int32_t* tok_index, const float* bias, const uint8_t* mask,
                           int B, int ntok, int C, int heads, int nc, int vol, float scale, float eps, const int32_t* tok_affine,
                           const pd_call_opts* opts, pd_stream_t stream);
/* One (CuboidSelfAttentionLayer, PositionwiseFFN) pair of StackCuboidSelfAttentionBlock.forward (cuboid_transformer.py:1147-1156:
 * x = x + attn(x); x = ffn(x) with the FFN's own residual; attention :812-966, FFN :182-208) in ONE launch, bf16 engine, GELU, cuboid
 * volume <= 16, no qkv bias, no attention mask, for units 256 (4 heads of 64, hidden 1024: every level-0 axial layer of the SEVIR-LR
 * denoiser) and units 512 (4 heads of 128, hidden 2048: every level-1 layer); in place allowed.  The rows of a wave (32 x 256 or
 * 16 x 512) stay in its registers from the first LayerNorm to the last residual: x is read once and written once
 * (csrc/pair_block.hip).  A wave works on 16-slot groups: one cuboid each, or pd_attn_ffn_pair_cuboids_per_group(vol) = 2 cuboids of
 * volume <= 8 side by side.
 *   wstream: 48 (units 256) / 192 (units 512) chunks of 32 KB = the four weight matrices as bf16 MFMA fragments in consumption order
 *            (prediff_amd/packing.py: pack_pair_block documents the layout);
 *   vecs:    LN1 gamma, beta, proj bias, LN2 gamma, beta, FFN-2 bias (units floats each), FFN-1 bias (hidden), then the (4, 16, 16) score
 *            table of a group: [head][query slot][key slot] = relative-position bias where both slots belong to the same cuboid, -inf
 *            everywhere else (padded slots, the group's other cuboid)  (pack_pair_vecs): 3584 / 6144 floats;
 *   tok_index [nc][vol] / tok_affine (HOST pointer, 4 ints, or NULL): as for pd_attn_block_fused_ex; one of them is required. */
int pd_attn_ffn_pair_supported(int C, int heads, int hidden, int vol, int act);
int pd_attn_ffn_pair_cuboids_per_group(int vol);
int pd_attn_ffn_pair(const float* x, float* out, const void* wstream, const float* vecs, const int32_t* tok_index,
                     const int32_t* tok_affine, int B, int ntok, int nc, int vol, int units, float scale, float eps_attn,
                     float eps_ffn, const pd_call_opts* opts, pd_stream_t stream);

/* The same pair for SMALL GRIDS (few trajectories per launch), units 512: two tile launches + two row sums that give every 64-row tile to FOUR workgroups,
 * each streaming a quarter of the weights -- (tile, head): LayerNorm-1 + that head's attention + its proj partial; a row sum
 * x' = x + b_proj + the four partials (in head order); (tile, quarter of the hidden units): LayerNorm-2 of x', that quarter's FFN partial;
 * a row sum of the four FFN partials (in order) into out.  x and vecs 16 B aligned.  Deterministic; the fp32 summation order differs from pd_attn_ffn_pair's (partials instead of one
 * running accumulator), so the two agree to fp32 round-off amplified by the 16-bit roundings downstream, not bit for bit.
 *   wffn_split: the FFN chunks of `wstream` in quarter-major order (prediff_amd/packing.py: pack_pair_ffn_split), 128 chunks of 32 KB;
 *   ws: caller workspace of pd_attn_ffn_pair_split_ws_floats(B, ntok, units) floats (2 x 4 partial slabs of x's size), 16 B aligned. */
int64_t pd_attn_ffn_pair_split_ws_floats(int B, int ntok, int units);
int pd_attn_ffn_pair_split(const float* x, float* out, const void* wstream, const void* wffn_split, const float* vecs,
                           const int32_t* tok_index, const int32_t* tok_affine, int B, int ntok, int nc, int vol, int units, float scale,
                           float eps_attn, float eps_ffn, float* ws, int64_t ws_floats, const pd_call_opts* opts, pd_stream_t stream);

/* PositionwiseFFN.forward alone (pre-norm LayerNorm -> Linear -> GELU -> Linear -> + x, cuboid_transformer.py:182-208) on the pair kernel's FFN
 * half (ABI 4): for blocks whose attention layer pd_attn_ffn_pair cannot take (cuboid volume > 16, masks: the full-resolution grid), units 256
 * (hidden 1024) or 512 (hidden 2048), GELU.  x, out: (rows, units) fp32 (may alias); wffn: the FFN chunks in the pair kernel's order
 * (packing.pack_pair_ffn_split(..., nsplit = 1)); vecs: the pair kernel's fp32 tables (packing.pack_pair_vecs; only LayerNorm-2, b1, b2 are read).
 * Rows are independent: any row count (a last partial group of 16 is masked). */
int pd_ffn_rows_supported(int C, int hidden, int act);
int pd_ffn_rows(const float* x, float* out, const void* wffn, const float* vecs, int64_t rows, int units, float eps,
                const pd_call_opts* opts, pd_stream_t stream);

/* The SEVIR pixel front end (DESIGN.md §7 "SEVIR pixel front end"; prediff_amd/sevir_io.py): raw VIL events to model frames and back.
 * pd_sevir_ingest: raw (N, H, W, T) uint8, layout NHWT (public SEVIR VIL: (N, 384, 384, 49)), to fp32 NTHWC frames with C = 1, one launch:
 *   LR frame t' = raw frame t' ft (T_lr = ceil(T / ft) of them); LR cell (h', w') = the maximum of the BYTES of the raw block
 *   [h' fh, h' fh + fh) x [w' fw, w' fw + fw) (save_downsampled_dataset, datasets/sevir/sevir_dataloader.py:460-467: block_reduce with
 *   np.max); value = scale * ((float)byte + offset), ONE fp32 add then ONE fp32 multiply, never an fma (preprocess_data_dict, :645;
 *   scale and offset arrive rounded to fp32 once).  H % fh == 0 and W % fw == 0.
 *   starts: nwin int32 LR frame indices ON THE DEVICE (the library cannot read the table: the caller checks 0 <= start <= T_lr - in_len -
 *   out_len; a window outside that range reads nothing and is written as zeros).  Sequence n * nwin + k is window k of event n:
 *   ctx (N nwin, in_len, H / fh, W / fw, 1) = LR frames [start_k, start_k + in_len), tgt (N nwin, out_len, H / fh, W / fw, 1) the out_len
 *   frames after them; tgt is NULL exactly when out_len = 0.  Every element of ctx and tgt is written exactly once; raw is only read, and
 *   nothing outside it is read whatever its alignment.  No synchronisation and no host reads: the launch can be captured.
 * pd_sevir_export: x (B, T, H, W, 1) fp32 to the VIL scale, v = x / scale - offset: ONE correctly rounded fp32 divide by the fp32 scale,
 *   then ONE fp32 subtract (process_data_dict_back, :679).  mode PD_SEVIR_F32: out is fp32 (B, T, H, W, 1) = v.  PD_SEVIR_U8_NTHW /
 *   PD_SEVIR_U8_NHWT: out is uint8 (B, T, H, W) / (B, H, W, T) = v clamped to [0, 255] and rounded half to even (torch.round); a NaN
 *   becomes 0.  out must not alias x.  Any alignment (16-byte accesses when both buffers allow them). */
enum pd_sevir_export_mode { PD_SEVIR_F32 = 0, PD_SEVIR_U8_NTHW = 1, PD_SEVIR_U8_NHWT = 2 };
int pd_sevir_ingest(const uint8_t* raw, const int32_t* starts, float* ctx, float* tgt, int N, int H, int W, int T, int ft, int fh, int fw,
                    int nwin, int in_len, int out_len, float scale, float offset, pd_stream_t stream);
int pd_sevir_export(const float* x, void* out, int64_t B, int T, int H, int W, float scale, float offset, int mode, pd_stream_t stream);

/* Optical-flow extrapolation (Lagrangian persistence; not in the reference; DESIGN.md §7 "Extrapolation baseline"; the definition is the
 * module docstring of prediff_amd/extrapolation.py).  fp32, fixed summation order: the same input gives the same bits.  No synchronisation
 * and no host reads: both calls can be captured.
 * pd_lk_motion: ctx (B, T, H, W, 1) fp32 -> motion (B, 2, H, W) fp32 = (v_y, v_x) in pixels per frame: pyramidal (levels), iterated (iters
 *   per level), damped Lucas-Kanade flow over the P = min(pairs, T - 1) newest frame pairs, window (2 radius + 1)^2.  T >= 2; H, W <= 512,
 *   divisible by 2^(levels - 1), the coarsest sides >= 4; 1 <= levels <= 8, 1 <= iters <= 64, 1 <= radius <= 9, P <= 16, damping > 0.
 *   ws: device workspace (4-byte aligned) of pd_lk_ws_bytes(...) bytes (-1: unsupported shape or options; host-only): the pyramid above
 *   level 0 and two flow buffers per level.  levels - 1 + levels * iters launches.
 * pd_advect: out (B, K, H, W, 1)[k - 1] = the frame sampled bilinearly at (y - k v_y, x - k v_x), k = 1 .. K, one launch.  frame: B images
 *   of H x W, frame_stride elements apart (>= H W: the last frame of a context is read in place); motion (B, 2, H, W), any values: a tap
 *   outside the frame reads `fill`, a coordinate that is not finite or further than 2^20 from the frame gives `fill`.  out aliases
 *   neither input. */
int64_t pd_lk_ws_bytes(int64_t B, int T, int H, int W, int levels, int iters, int radius, int pairs);
int pd_lk_motion(const float* ctx, float* motion, int64_t B, int T, int H, int W, int levels, int iters, int radius, float damping, int pairs,
                 void* ws, int64_t ws_bytes, pd_stream_t stream);
int pd_advect(const float* frame, const float* motion, float* out, int64_t B, int K, int H, int W, int64_t frame_stride, float fill,
              pd_stream_t stream);

/* Stochastic extrapolation (STEPS; S-PROG without noise; not in the reference; DESIGN.md §7 "Stochastic extrapolation"; the definition is
 * the module docstring of prediff_amd/steps.py, whose step numbers are used here).  fp32 fields, fp64 statistics in a fixed order, no
 * atomics: the same input gives the same bits.  No synchronisation and no host reads: every call can be captured.
 * Frames: H and W are 2^a or 3 * 2^a, >= 8, H W <= 16384 (one complex frame stays in LDS); 2 <= levels <= floor(log2(max(H, W))) - 1;
 * ar_order 1 or 2; ctx (B, T, H, W, 1) with T >= ar_order + 1; motion (B, 2, H, W); bands (levels, H, W): real, even weights
 * (prediff_amd.steps.steps_bands).  ws: device workspace, 8-byte aligned.
 * pd_steps_ws_bytes: what the workspace of B sequences and M members holds (-1: unsupported; host-only).  M = 0 is what pd_steps_analyse
 *   alone needs; pd_steps_evolve needs the size of its own M and the workspace pd_steps_analyse filled.
 * pd_steps_analyse (steps 0 .. 5, one workgroup per sequence): mu, sigma (B, levels) of the cascade of the last frame (a dead level
 *   reports sigma 0), phi (B, levels, 3) = (phi1, phi2, phi0), gamma (B, levels, 2); the normalised levels of the two newest Lagrangian
 *   frames and the noise filter P go to the workspace.
 * pd_steps_evolve (steps 6 .. 8, one workgroup per (member, sequence), looping over the leads): noise (M, B, K, H, W) standard
 *   normal, or NULL for zero innovations -> R (M, B, K, H, W), the recomposed Lagrangian fields.  mu / sigma / phi: what pd_steps_analyse
 *   wrote.  Two cascade levels of ONE member travel as one complex frame (an odd `levels` leaves the last pair half empty); members are
 *   never packed with each other, so a member alone, with its own noise, gives the bits it gives inside any ensemble.  R aliases no input.
 * pd_steps_finish (step 9, one workgroup per (member, sequence, lead)): mask (0 none, 1 "obs"), match (0 none, 1 "mean"), the threshold
 *   cut and pd_advect's rule at the single lead k with fill 0: R (M, B, K, H, W) -> out (M, B, K, H, W, 1).  out aliases no input. */
int64_t pd_steps_ws_bytes(int64_t B, int M, int H, int W, int levels, int ar_order);
int pd_steps_analyse(const float* ctx, const float* motion, const float* bands, int64_t B, int T, int H, int W, int levels, int ar_order,
                     float threshold, float* mu, float* sigma, float* phi, float* gamma, void* ws, int64_t ws_bytes, pd_stream_t stream);
int pd_steps_evolve(const float* noise, const float* bands, const float* mu, const float* sigma, const float* phi, int M, int64_t B, int K,
                    int H, int W, int levels, int ar_order, float* R, void* ws, int64_t ws_bytes, pd_stream_t stream);
int pd_steps_finish(const float* ctx, const float* motion, const float* R, float* out, int M, int64_t B, int T, int K, int H, int W,
                    float threshold, int mask, int match, pd_stream_t stream);

/* Growth / decay extrapolation (ANVIL, deterministic; not in the reference; DESIGN.md §7 "Growth and decay extrapolation"; the definition
 * is the module docstring of prediff_amd/anvil.py, whose step numbers are used here).  An ARI(p, 1) model of the cascade levels in
 * Lagrangian coordinates whose AR parameters are estimated per pixel in a Gaussian window.  fp32 fields, the one fp64 sum in a fixed
 * order, no atomics: the same input gives the same bits.  No synchronisation and no host reads: every call can be captured.
 * Frames, levels and bands as pd_steps_*; ar_order p is 1 or 2; ctx (B, T, H, W, 1) with T >= p + 2; motion (B, 2, H, W).
 * window: the 2 radius + 1 fp32 weights g[-radius .. radius] of step 6 on the device, 1 <= radius <= 96; window_sum_sq: W0 of step 7,
 * (sum_d g[d])^2, which the host knows.  ws: device workspace, 16-byte aligned; phi, gamma and R are 16-byte aligned too.
 * pd_anvil_ws_bytes: what the workspace of B sequences holds (-1: unsupported; host-only).
 * pd_anvil_analyse (steps 2 .. 8): one launch of B x 2 workgroups for the forward spectra of the packed Lagrangian frames (and mean(A_0^2)),
 *   one of B x levels workgroups for the levels, their differences, the windowed moments and the per-pixel Yule-Walker solve:
 *   phi (B, levels, 2, H, W) = (phi1, phi2), gamma (B, levels, 2, H, W) = the clamped (gamma_1, gamma_2); Y_l0 and D_l0 .. D_lp stay in
 *   the workspace.
 * pd_anvil_evolve (step 9, pointwise): phi and the workspace pd_anvil_analyse filled -> R (B, K, H, W), the recomposed Lagrangian
 *   fields, lead k at [:, k - 1].  R aliases no input.  Step 10 is pd_steps_finish with M = 1, mask = 0, match = 0. */
int64_t pd_anvil_ws_bytes(int64_t B, int H, int W, int levels, int ar_order);
int pd_anvil_analyse(const float* ctx, const float* motion, const float* bands, const float* window, int radius, double window_sum_sq,
                     int64_t B, int T, int H, int W, int levels, int ar_order, float* phi, float* gamma, void* ws, int64_t ws_bytes,
                     pd_stream_t stream);
int pd_anvil_evolve(const float* phi, int64_t B, int K, int H, int W, int levels, int ar_order, float* R, const void* ws, int64_t ws_bytes,
                    pd_stream_t stream);

/* SEVIRSkillScore.update (datasets/sevir/evaluation.py:193-239): hits / misses / false alarms of (pred / divisor) vs
 * (target / divisor) at every threshold (>=, NaN in either input counts nowhere), accumulated into counts[thr][t][3]
 * (int64, keep_seq) or counts[thr][3].  Tensors are (outer, T, inner) fp32 in [0,1]; divisor = fp32(1/255). */
int pd_sevir_skill_counts(const float* pred, const float* target, const float* thresholds, int nthr, float divisor,
                          long long* counts, int64_t outer, int T, int64_t inner, int keep_seq, pd_stream_t stream);

/* SEVIRSkillScore.update with preprocess_type "sevir_pool{s}" (datasets/sevir/evaluation.py:220-231): pred and target are max-pooled over
 * (H, W) with kernel = stride = pool for each (N, T, C) (floor mode; a NaN in a window makes the cell NaN), divided by divisor, then counted
 * as pd_sevir_skill_counts does into the same counts[thr][t][3] (keep_seq) or counts[thr][3].  sizes: host int64[5] = N, T, H, W, C;
 * pred_strides / target_strides: host int64[5], the element strides of those axes (any layout is read in place; a missing axis has
 * size 1).  nthr <= 8. */
int pd_sevir_skill_counts_pooled(const float* pred, const float* target, const float* thresholds, int nthr, float divisor,
                                 long long* counts, const int64_t* sizes, const int64_t* pred_strides, const int64_t* target_strides,
                                 int pool, int keep_seq, pd_stream_t stream);

/* Ensemble verification (not in the reference): ens holds M members of target's shape (1 <= M <= 512), both preprocessed like
 * pd_sevir_skill_counts_pooled (pool = 1: no pooling).  A pooled pixel is valid when the target and all members are non-NaN there; per
 * valid pixel of step t (t = 0 unless keep_seq) it adds 1 to n_valid[t] (int64), (c - M o)^2 to brier[thr][t] (int64, exact; c = #{x_i >=
 * thr}, o = [y >= thr]) and, in fp64, sum_i |x_i - y| to sums[0][t], sum_ij |x_i - x_j| to sums[1][t], (mean - y)^2 to sums[2][t] and
 * sum_i (x_i - mean)^2 / (M - 1) (0 for M = 1) to sums[3][t].  The fp64 sums are reduced in a fixed order (bit-reproducible).
 * sizes: host int64[5] = N, T, H, W, C; ens_strides: host int64[6] = member, N, T, H, W, C strides; target_strides: host int64[5].
 * ws: device workspace of pd_ensemble_score_ws_doubles(M, sizes, pool) doubles (-1: unsupported M / sizes). */
int64_t pd_ensemble_score_ws_doubles(int M, const int64_t* sizes, int pool);
int pd_ensemble_score_update(const float* ens, const float* target, const float* thresholds, int nthr, float divisor, int M,
                             const int64_t* sizes, const int64_t* ens_strides, const int64_t* target_strides, int pool, int keep_seq,
                             long long* n_valid, long long* brier, double* sums, double* ws, int64_t ws_doubles, pd_stream_t stream);

/* Frame scores of test_step (train_sevirlr_prediff.py:937-965: torchmetrics' MeanSquaredError, MeanAbsoluteError and the default
 * StructuralSimilarityIndexMeasure): pred holds M members of target's shape (1 <= M <= 512), both fp32, read in place.  Per step t (t = 0
 * unless keep_seq), in fp64 and in a fixed order (bit-reproducible): sums[0][t] += sum (p - t)^2, sums[1][t] += sum |p - t|,
 * sums[2][t] += sum over the (member, n) frames of the frame's SSIM -- 11 x 11 Gaussian window (sigma 1.5), c1 = (0.01 R)^2,
 * c2 = (0.03 R)^2, variances clamped at 0, mean over the C (H - 10)(W - 10) windows inside the frame; counts[0][t] += elements,
 * counts[1][t] += frames (int64).  No NaN masking.  R = data_range, or, when range_buf (device, 2 floats) is not NULL, the call first
 * writes [max - min of pred, max - min of target] there and uses R = the larger of the two (NaN if either tensor holds one).
 * sizes: host int64[5] = N, T, H, W, C (H, W >= 11, else PD_ERR_ARG); pred_strides: host int64[6] = member, N, T, H, W, C element
 * strides; target_strides: host int64[5].  ws: device workspace of pd_frame_score_ws_doubles(M, sizes) doubles (-1: unsupported). */
int64_t pd_frame_score_ws_doubles(int M, const int64_t* sizes);
int pd_frame_score_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                          const int64_t* target_strides, float data_range, float* range_buf, int keep_seq, double* sums,
                          long long* counts, double* ws, int64_t ws_doubles, pd_stream_t stream);

/* Radially averaged power spectra of forecast / observation pairs (the RAPSD diagnostic of the nowcasting literature, with the spectral
 * coherence): pred holds M members of target's shape (1 <= M <= 512), both fp32, read in place; every (member, n, t, c) plane of pred is
 * paired with the (n, t, c) plane of target.  With P, T the 2-D DFTs of the two H x W frames of a pair (after the window: 0 none,
 * 1 periodic Hann) and s = 1 / (H W), per radial bin b and step t (t = 0 unless keep_seq), in fp64 and in a fixed order
 * (bit-reproducible): sums[0][t][b] += s |P|^2, sums[1][t][b] += s |T|^2, sums[2][t][b] += s Re(P conj T) over the cells of the bin;
 * frames[t] += pairs (int64).  No NaN masking.  The bins are the caller's: cell_order (device int32, the kept cells ky W + kx sorted by
 * bin) and bin_start (device int32[nb + 1]), nb = max(H, W) / 2 + 1 (prediff_amd/spectrum.py: spectrum_bins).
 * sizes: host int64[5] = N, T, H, W, C; H and W are 2^a or 3 * 2^a, 8 .. 512 (else PD_ERR_ARG, the message names the side).
 * pred_strides: host int64[6] = member, N, T, H, W, C element strides; target_strides: host int64[5].  ws: device workspace, 8-byte
 * aligned; pd_spectrum_ws_bytes(M, sizes) is what holds every pair of the call, capped at 256 MiB (-1: unsupported shape, host-only);
 * a smaller workspace (at least pd_spectrum_ws_bytes(1, {1, 1, H, W, 1})) makes the call run in several chunks of pairs. */
int64_t pd_spectrum_ws_bytes(int M, const int64_t* sizes);
int pd_spectrum_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                       const int64_t* target_strides, const int* cell_order, const int* bin_start, int nb, int window, int keep_seq,
                       double* sums, long long* frames, void* ws, int64_t ws_bytes, pd_stream_t stream);

/* Object-based verification (not in the reference): connected-component labelling of frames, the per-object table, and SAL (Wernli et al.
 * 2008, Mon. Wea. Rev. 136, 4470).  A frame is one (n, t) image of H x W fp32 pixels, C = 1, 1 <= H, W <= 128 (the label image lives in
 * LDS; else PD_ERR_ARG, the message names the limit), read in place.  Object pixels: v >= thr and v > 0, with thr = threshold when
 * use_threshold != 0, else the fp32 product thr_factor * max(frame) of that frame (NaN, hence no object, when the frame holds a NaN).
 * Objects: the components of that mask under connectivity 4 or 8 that have at least min_pixels pixels, numbered 1, 2, ... in raster order
 * of their first pixel.
 * pd_objects_label: sizes / strides: host int64[5] = N, T, H, W, C sizes and element strides.  records: device, N T records of 9
 * doubles (pd_objects_ws_bytes(0, sizes) bytes): D = sum v / (H W), sum v, sum v row, sum v col (all pixels); sum R_n^2 / P_n, sum R_n,
 * sum R_n |x - x_n| (objects: mass R, peak P, centroid x_n, x the mass centre of the frame); the object count; flags (1: the frame holds a
 * non-finite pixel -- it gets labels and a count, and zero object sums).  labels: NULL or device int32 (N, T, H, W), 0 = background.
 * table: NULL or device fp64 (N, T, max_objects, 6), row k - 1 of object k: mass, peak, area, row centroid, col centroid, first-pixel
 * index row W + col; objects beyond max_objects are left out of the table only, and rows beyond the count are not written.
 * Labels, counts, areas and first-pixel indices are exact; the object sums are added as integers (two 40-bit fixed-point limbs relative
 * to the frame maximum: exact for pixels >= 2^-57 of it) and so is every record: the same frame gives the same bits.
 * pd_sal_update: pred holds M members of target's shape (1 <= M <= 512; pred_strides: host int64[6] = member, N, T, H, W, C;
 * target_strides: host int64[5]); the target's frames are labelled once.  Per (member, n, t) pair and step t (t = 0 unless keep_seq), in
 * fp64 and in a fixed order: a pair with a flagged frame adds 1 to counts[1][t] and nothing else; every other pair adds 1 to counts[0][t],
 * its object counts to counts[6][t] (pred) and counts[7][t] (target), and, where defined, A = (D_F - D_O) / ((D_F + D_O) / 2) to
 * sums[1][t] (|A| to sums[6][t], 1 to counts[3][t]; defined when D_F + D_O != 0), S = (V_F - V_O) / ((V_F + V_O) / 2), V = sum R_n^2 / P_n /
 * sum R_n, to sums[0][t] (|S| to sums[5][t], 1 to counts[2][t]; both frames have an object), L1 = |x_F - x_O| / d to sums[2][t] (1 to
 * counts[4][t]; both frames have mass; d = sqrt((H - 1)^2 + (W - 1)^2) > 0), L2 = 2 |r_F - r_O| / d, r = sum R_n |x - x_n| / sum R_n, to
 * sums[3][t] and L1 + L2 to sums[4][t] (1 to counts[5][t]; objects and mass in both).  sums: device fp64 [7][T'], counts: device int64
 * [8][T'].  ws: device workspace of pd_objects_ws_bytes(M, sizes) bytes, 8-byte aligned (-1: unsupported M / sizes). */
int64_t pd_objects_ws_bytes(int M, const int64_t* sizes);
int pd_objects_label(const float* frames, const int64_t* sizes, const int64_t* strides, float threshold, int use_threshold,
                     float thr_factor, int connectivity, int min_pixels, double* records, int* labels, double* table, int max_objects,
                     pd_stream_t stream);
int pd_sal_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                  const int64_t* target_strides, float threshold, int use_threshold, float thr_factor, int connectivity, int min_pixels,
                  int keep_seq, double* sums, long long* counts, void* ws, int64_t ws_bytes, pd_stream_t stream);

/* Probability matching (not in the reference; DESIGN.md §7 "Probability matching"; the definitions are the module docstring of
 * prediff_amd/probability_matching.py).  A frame is n = H W contiguous fp32 pixels, 1 <= H, W and n <= 16384 (it is sorted in LDS).  ORDER:
 * ascending by the exact fp32 value (compared as integer keys: denormals are never flushed; -0.0 ties with +0.0), ties by ascending pixel
 * index.  Every result is a selection of input values: exact, no atomics, the same inputs give the same bits.  No synchronisation and no
 * host reads: every call can be captured.  Outputs alias no input and not the workspace.
 * pd_pm_ws_bytes: the workspace of an op (host-only; -1: unsupported): op 0 pd_rank_frames (needs none: 0), op 1 pd_cdf_match with
 *   `frames` REFERENCE frames: their sorted keys and flags, align8(4 frames n) + align8(4 frames); op 2 pd_pmm with M members of `frames`
 *   (b, t) frames: two buffers of the pooled keys, 2 align8(4 frames M n).  frames (M) n <= 2^31.
 * pd_rank_frames: x (frames, n) -> order int32 (frames, n), sorted fp32 (frames, n), sorted[r] = x[order[r]] (the original bits).  A frame
 *   with a non-finite pixel gets order -1 and sorted NaN throughout.
 * pd_cdf_match: x (lead, B, T, n), ref (B, ref_T, n) with ref_T = T or 1 (one reference frame for every t) -> out shaped like x.  Per
 *   frame, s = the sorted reference frame (-0.0 read as +0.0; sorted once per reference frame); with use_threshold, n_x = #{x > threshold}
 *   and s[r] <- min(s[r], threshold) for r < n - n_x; out[order_x[r]] = s[r].  A non-finite pixel in the frame of x or of ref makes the
 *   output frame NaN.  ws: pd_pm_ws_bytes(1, 1, B ref_T, H, W) bytes, 8-byte aligned.
 * pd_pmm: ens (M, frames, n), 1 <= M <= 512 -> out (frames, n).  Per frame: mean = float(sum_m double(ens[m]) / M) (fp64 sum in member
 *   order, fp64 division, one rounding); P = the M n member values in ascending order (-0.0 read as +0.0);
 *   out[order_mean[r]] = P[r M + M / 2].  A non-finite pixel in any member's frame makes the output frame NaN.
 *   ws: pd_pm_ws_bytes(2, M, frames, H, W) bytes, 8-byte aligned. */
int64_t pd_pm_ws_bytes(int op, int M, int64_t frames, int H, int W);
int pd_rank_frames(const float* x, int64_t frames, int H, int W, float* sorted, int* order, pd_stream_t stream);
int pd_cdf_match(const float* x, const float* ref, int64_t lead, int64_t B, int T, int ref_T, int H, int W, float threshold,
                 int use_threshold, float* out, void* ws, int64_t ws_bytes, pd_stream_t stream);
int pd_pmm(const float* ens, int M, int64_t frames, int H, int W, float* out, void* ws, int64_t ws_bytes, pd_stream_t stream);

/* Distance-map verification (not in the reference; Gilleland 2011 / 2017; the definitions are the module docstring of
 * prediff_amd/distance_score.py).  A frame is one (n, t) image of H x W fp32 pixels, C = 1, 1 <= H, W <= 128 (the maps of a frame live in
 * LDS; else PD_ERR_ARG, the message names the limit), read in place.  Event set of a threshold: { s : v[s] / divisor >= thr } in fp32
 * (IEEE division, as pd_sevir_skill_counts; divisor 1 compares the raw value; a NaN is never an event).  d2[s]: the squared Euclidean
 * distance from pixel s to the nearest event of its frame, an exact integer <= 32258; 2^31 - 1 everywhere in a frame without events.
 * pd_distance_map: sizes / strides: host int64[5] = N, T, H, W, C sizes and element strides (no negative stride) -> d2, device int32
 *   (N, T, H, W), which must not alias the frames.
 * pd_distance_update: pred holds M members of target's shape (1 <= M <= 512; pred_strides: host int64[6] = member, N, T, H, W, C;
 *   target_strides: host int64[5]); thresholds: HOST float[K], 1 <= K <= 8.  Every frame is read once for all K thresholds and the target's
 *   maps are made once for all members.  Per (member, n, t) pair, threshold k and step t (t = 0 unless keep_seq), with F / O the event sets
 *   of pred / target and d = sqrt(double(d2)): a pair with a non-finite pixel in either frame adds 1 to counts[1][k][t] and nothing else;
 *   every other pair adds 1 to counts[0][k][t], |F| to counts[4][k][t] and |O| to counts[5][k][t]; where F and O are both non-empty, 1 to
 *   counts[2][k][t], mean over O of d_F to sums[0][k][t], mean over F of d_O to sums[1][k][t] and
 *   sqrt(max(max over O of d2_F, max over F of d2_O)) (the maximum of integers) to sums[2][k][t]; Baddeley's
 *   sqrt(sum over all pixels of (w(d_F) - w(d_O))^2 / (H W)) to sums[3][k][t] and 1 to counts[3][k][t], with w(d) = min(d, cutoff) and w = cutoff
 *   for an empty set when use_cutoff != 0 (cutoff positive and finite; defined for every such pair), else w(d) = d where F and O are both
 *   non-empty.  sums: device fp64 [4][K][T'], counts: device int64 [6][K][T'].  All sums are fp64, added in a fixed order, with no atomics: the
 *   same inputs give the same bits.  ws: device workspace of pd_distance_ws_bytes(M, K, sizes) bytes (host-only; -1: unsupported M / K /
 *   sizes), 16-byte aligned, aliasing neither an input nor the state. */
int64_t pd_distance_ws_bytes(int M, int K, const int64_t* sizes);
int pd_distance_map(const float* frames, const int64_t* sizes, const int64_t* strides, float threshold, float divisor, int* d2,
                    pd_stream_t stream);
int pd_distance_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                       const int64_t* target_strides, const float* thresholds, int K, float divisor, int use_cutoff, double cutoff,
                       int keep_seq, double* sums, long long* counts, void* ws, int64_t ws_bytes, pd_stream_t stream);

/* Intensity-scale verification (not in the reference; Casati, Ross and Stephenson 2004; Casati 2010; the definitions are the module
 * docstring of prediff_amd/scale_score.py).  Frames, event sets and limits are those of the distance block above (C = 1, 1 <= H, W <= 128,
 * no negative stride, read in place; a NaN is never an event).  The 0 / 1 event field of a frame sits at the top-left corner of an S x S
 * field of zeros, S = 2^n the smallest power of two >= max(H, W, 2) (n = 1 .. 7).  Q_l(A), l = 0 .. n: the sum over the 2^l x 2^l blocks
 * of that field of (block sum of A)^2, an exact integer <= 4^(n + l) <= 2^28.  Everything after the event test is integer arithmetic.
 * pd_scale_energy: sizes / strides: host int64[5] -> q_out, device int64 [N T][8]: Q_l of the event field of every frame at one
 *   threshold, zero for l > n; q_out must not alias the frames.
 * pd_scale_update: operands as pd_distance_update (thresholds: HOST float[K], 1 <= K <= 8; 1 <= M <= 512).  Every frame is read once for
 *   all K thresholds and the target's event planes are made once for all members.  With I_F / I_O the event fields of pred / target and
 *   Z = I_F - I_O, per (member, n, t) pair and step t (t = 0 unless keep_seq): a pair with a non-finite pixel in either frame adds 1 to
 *   counts[1][t] and nothing else; every other pair adds 1 to counts[0][t] and Q_l(I_F), Q_l(I_O), Q_l(Z) to energy[0 / 1 / 2][k][l][t] for
 *   l = 0 .. n (levels above n are not touched).  energy: device int64 [3][K][8][T'], counts: device int64 [2][T'].  No atomics; integer
 *   sums in a fixed order.  ws: device workspace of pd_scale_ws_bytes(M, K, sizes) bytes (host-only; -1: unsupported M / K / sizes),
 *   16-byte aligned, aliasing neither an input nor the state. */
int64_t pd_scale_ws_bytes(int M, int K, const int64_t* sizes);
int pd_scale_energy(const float* frames, const int64_t* sizes, const int64_t* strides, float threshold, float divisor, long long* q_out,
                    pd_stream_t stream);
int pd_scale_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                    const int64_t* target_strides, const float* thresholds, int K, float divisor, int keep_seq, long long* energy,
                    long long* counts, void* ws, int64_t ws_bytes, pd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Fréchet video distance (evaluation/fvd/): the pieces of the I3D feature engine that are not pd_igemm, and the feature moments.
 * ------------------------------------------------------------------------------------------------- */
/* I3DWrapper.preprocess (evaluation/fvd/torchmetrics_wrap.py:33-65) with the frame handling of FrechetVideoDistance.update (:223-233) in
 * one launch.  x: fp32 frames read in place; sizes: host int64[5] = N, T, H, W, C (C = 1 is read as three equal channels, else C = 3);
 * strides: host int64[5], element strides of those axes.  normalize != 0: x / 255 first; auto_t != 0: every frame twice
 * (repeat_interleave along T: T2 = 2 T frames, else T2 = T).  Bilinear resize (align_corners = False, no antialias) of the short side to 224
 * and the other side to ceil(side * 224 / short side), centre crop to 224 x 224 at offsets (size - 224) / 2, then 2 x - 1
 * (rescale != 0; rescale == 0 leaves the value as it is: frames that are in [-1, 1] already, InceptionI3d.forward).
 * out (/ out_lo: the low halves of the hi/lo engine, else NULL): the stem convolution's A operand, (N, T2, 224, 112, 64) 16-bit rows: the
 * im2col along W at the stem's stride -- column 3 dw + c of row (n, t, y, ow) = frame[y][2 ow - 2 + dw][c] for dw = 0..6, zero outside the
 * frame and in columns 21..63 (the stem then is a KT = 7, KH = 7, KW = 1 launch, strides (2, 2, 1), front pads (pt, 2, 0)).
 * out_f32: NULL, or (N, T2, 224, 224, 3) fp32, the preprocessed frames before the operand rounding. */
int pd_i3d_preprocess(const float* x, const int64_t* sizes, const int64_t* strides, int normalize, int auto_t, int rescale, pd_bf16* out,
                      pd_bf16* out_lo, float* out_f32, const pd_call_opts* opts, pd_stream_t stream);

/* MaxPool3dSamePadding (evaluation/fvd/pytorch_i3d.py:8-35) on channels-last fp32 x (B, T, H, W, C) rows of ld_in floats.  Per dimension
 * pad = max(k - s, 0) if size % s == 0 else max(k - size % s, 0), front pad = pad / 2, output size (size + pad - k) / s + 1 (= ceil(size / s)).
 * The padding holds the VALUE 0 and takes part in the max (the reference pads with zeros, then pools).  k >= s per dimension; C, ld_in,
 * ld_out, ld_outb multiples of 4.  Writes fp32 rows (out_f32, ld_out) and / or 16-bit operand rows (outb[, outb_lo], ld_outb; columns
 * >= C are not written). */
int pd_maxpool3d_same(const float* x, float* out_f32, pd_bf16* outb, pd_bf16* outb_lo, int B, int T, int H, int W, int C, int ld_in,
                      int kt, int kh, int kw, int st, int sh, int sw, int ld_out, int ld_outb, const pd_call_opts* opts, pd_stream_t stream);

/* The end of InceptionI3d.forward (pytorch_i3d.py:301-306): AvgPool3d((2, 7, 7), stride 1) -> logits 1x1x1 convolution + bias -> mean over
 * the T - 1 remaining time positions.  x (B, T, HW, C) fp32 channels last with the whole HW map inside the pool window (HW = 49), T >= 2;
 * W (N, C) fp32 row major, bias (N) or NULL; pooled: (B, C) floats of workspace; out (B, N) fp32.  The pool commutes with the linear
 * layer, so the frames are averaged first (weights (t >= 1) + (t <= T - 2) over 2 HW (T - 1)). */
int pd_i3d_head(const float* x, const float* W, const float* bias, float* pooled, float* out, int B, int T, int HW, int C, int N,
                pd_stream_t stream);

/* FrechetVideoDistance.update's state (torchmetrics_wrap.py:241-247): f (n, d) fp32 rows of ld floats; sum[j] += sum_k f[k][j] and
 * cov_sum[i][j] += sum_k f[k][i] f[k][j] in fp64, k ascending per entry (no atomics: the same inputs give the same bits).
 * n >= 1, d <= 4096. */
int pd_feature_moments_update(const float* f, int64_t n, int d, int ld, double* sum, double* cov_sum, pd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PREDIFF_HIP_H */
