// pd_igemm, halo-staged Conv3d 3x3x3: the 256 x 256 x 64 eight-wave kernel of igemm256.hip with the A operand staged ONCE per input frame.
//
// igemm256_kernel walks K tap-major and stages a fresh 256 x 64 A tile for every K-tile.  For a stride-1, pad-1, un-upsampled 3x3x3
// convolution on 16 x 16 frames a 256-row tile IS one output frame, and the A rows of the nine (kh, kw) taps of one (channel chunk,
// temporal tap) are the same 18 x 18 input pixels (frame + spatial ring) at shifted positions: nine K-tiles staged 9 x 32 KB of A out of
// one 41.5 KB halo.  This kernel walks K as  channel chunk (64) -> temporal tap kt -> (kh, kw),  stages the halo of a (chunk, kt) group
// once and reads the A fragments of the nine K-tiles of the group out of it at a row shift of kh * 18 + kw.  DMA pieces per wave and
// K-tile: 4 (W) + 5.25 / 9 (halo) = 4.6 instead of 8.  The tile, the eight waves, the two-phase MFMA schedule, the wave-row stagger, the W
// stream (rows, swizzle, two K-tile buffers, issued two K-tiles ahead in phase B) and the epilogue are those of igemm256_kernel<2, 8>.
//
// Halo layout in LDS: eight PLANES, one per 16-B k-slot s of the 128-B channel chunk; plane s holds the 16 B of halo row r (= hr * 18 + hc,
// 324 rows, 336 allocated) at  s * PLANE + r * 16,  PLANE = 336 * 16 = 21 * 256 B.  The fragment read of lane (l16, lg) for row tile i
// (= image row oh = 8 * wave row + i), tap (kh, kw) and k-step ks is the 16 B at
//      ((oh + kh) * 18 + kw + l16) * 16  +  (4 ks + lg) * PLANE
// -- one per-lane base register and a COMPILE-TIME offset per (i, kh, kw, ks): no address arithmetic in the loop.  Banks (ds_read_b128 is
// served in four groups of 16 lanes, each group holding every l16 once with lg differing between its lanes): PLANE is a multiple of the
// 256-B bank row, so a lane's four banks are 4 * ((R + l16) mod 16) + 0..3 whatever its lg -- 16 consecutive halo rows R .. R + 15 hit 16
// different bank quads for EVERY shift R: conflict-free for all nine taps.  (A row-major halo with the (row >> 1) & 7 XOR swizzle of the W
// tile is conflict-free only for R % 4 == 0: rows r and r + 2 of one aligned group of four collide when they sit on either side of the
// l16 = 3 | 4 or 11 | 12 boundary of a lane group.)
// A DMA instruction of a wave fills 64 consecutive 16-B cells of that layout (1 KB; each lane names its own source pixel): a halo is 42
// pieces, wave w issues pieces w, w + 8, ..., w + 32 and waves 0 / 1 also pieces 40 / 41.  The spatial ring, the 12 spare rows of a plane
// and (dense loop) out-of-range frames come out of the descriptor's bounds check as zeros.
//
// Schedule of K-tile j = 0 .. 8 of group g (k = 9 g + j; halo g in halo buffer g & 1, W tile k in W buffer k & 1):
//   phase A: fragment reads (W column tiles 0-3, A row tiles 0-3); j = 1 .. 5: one halo piece of group g + 1 (j = 1: first the extra piece)
//   phase B: A row tiles 4-7; the four W pieces of K-tile k + 2; counted vmcnt: everything but this K-tile's own pieces has landed
// Hazards: halo buffer (g + 1) & 1 was last read in phase B of the last K-tile of group g - 1 and is refilled from K-tile 1 of group g; its
// last piece is issued in K-tile 5 and retired by the vmcnt(4) of K-tile 6, every wave passes that wait and two workgroup barriers before
// any wave reads the buffer.  Waves 0 / 1 issue their extra piece FIRST, so it is older than every piece a counted wait must retire:
// vmcnt(n) leaves the n YOUNGEST operations in flight, and those are the same for all eight waves.  W: as in igemm256_kernel.
// A kt whose input frame lies outside the sample is left out as a whole group (A and W): the tile-wide tap skipping of igemm256_kernel;
// debug_flags bit 8 keeps the dense loop (zero halos streamed, identical bits).
//
// Border-row skip (conv3d_halo_kernel<L, true>, the default; debug_flags bit 256 launches <L, false>, the dense MFMA schedule, for A/B runs
// and as the tests' reference).  A row tile is one image row, so the row tile of image row 0 reads, for the three taps with kh = 0, halo row
// 0 and nothing else: sixteen cells of the zero ring, whatever kw.  Likewise image row 15 and halo row 17 at kh = 2.  Those row tiles are
// left out of their phase -- both k-steps against all four column tiles, 8 of the phase's 32 MFMAs, and the two LDS reads of the A fragment:
//   wave row 0: local row tile 0 in phase A of K-tiles j = 0, 1, 2 (kh = j / 3 is a compile-time value in the unrolled loop);
//   wave row 1: local row tile 7 (local tile 3 of phase B) in phase B of K-tiles j = 6, 7, 8.
// 24 of a wave's 576 MFMAs per group (4.17 %).  The two wave rows leave out different tiles, so the loop is compiled once per wave row and
// entered through one scalar branch on the (wave-uniform) wave row: no test inside the loop, the code of the kernel grows by the two extra
// copies of the nine-K-tile body (112.6 -> 128.9 KB, most of either being the epilogue).  Every barrier, DMA piece and vmcnt constant is in
// both copies exactly where it was: no VMEM instruction is added or removed per wave, so the hazard analysis above holds unchanged; in a
// shortened section six accumulators (not eight) lie between two MFMAs on the same one.
// Exactness: a product left out is 0 * w.  An accumulator starts at +0 and can never become -0 ((+0) + (+-0) = +0 in round-to-nearest), so
// for finite weights adding +-0 changes no bit: the stored output is bit-identical to the dense schedule's.  With an Inf or NaN WEIGHT the
// dense schedule makes 0 * w = NaN in those border rows and this one does not -- the property the whole-group temporal skip above already has.
//
// Level 1 (conv3d_halo_kernel<1>, tile 11): 8 x 8 frames.  A 256-row tile is FOUR frame slots (frames 4 tm .. 4 tm + 3 of the batch; T need
// not be a multiple of 4, so a tile may hold the last frames of one sample and the first of the next), and a group's halo is the four input
// frames of its kt.  Everything above holds with these differences:
//  - Halo cell of (frame slot f, halo row hr, halo column hc), hr, hc = 0 .. 9:  base(f) + hr * 9 + hc.  Row pitch 9: column 9 of a row IS
//    column 0 of the next (both zero); row 9 of a frame runs into row 0 of the next (both zero).  base = 0, 88, 169, 257 (a frame needs 81
//    cells up to its neighbour and reaches 91): 348 cells, 352 allocated, 44 pieces, waves 0-3 issue a sixth.
//  - An MFMA row tile is NOT two neighbouring image rows of one frame: at any pitch that leaves room for the zero column, their cells
//    R .. R + 7 and R + pitch .. R + pitch + 7 share a bank quad.  Row tile i of wave row wr is image row i of frame slots 2 wr and 2 wr + 1:
//    lane l16 reads pixel (i, l16 & 7) of slot 2 wr + (l16 >> 3), and base(2 wr + 1) - base(2 wr) = 88 = 8 mod 16, so the 16 lanes of a group
//    hit quads R .. R + 7 and R + 8 .. R + 15: conflict-free for all nine shifts.  The epilogue undoes the permutation when it writes the
//    accumulators to its LDS slab (MFMA row rho of row tile i -> slab row (rho >> 3) * 64 + i * 8 + (rho & 7)); the slab a wave row hands to
//    igemm_epilogue is 128 consecutive output rows as before.
//  - Zero fill is per frame slot: a temporal tap can be in range for one slot and out of range for its neighbour (another sample), so each
//    staging lane carries its cell's slot and tests it against the group's four-bit validity mask; slots past the last frame (B * T not a
//    multiple of 4) are never valid, and the epilogue stores no row >= M.
//  - No group is skipped (all four slots are out of range only when T = 1): debug_flags bit 8 changes nothing.
//  - Border-row skip: row tile i is image row i of BOTH frame slots of the wave row, so row tile 0 at kh = 0 (halo row 0 of both slots) and
//    row tile 7 at kh = 2 (halo row 9) are all-zero in both wave rows: a compile-time condition, one copy of the loop, 48 of a wave's 576
//    MFMAs per group (8.33 %).  (A slot whose temporal tap is out of range is zero as a whole, but only for that slot and that tile.)
#include <algorithm>
#include "common.h"
#include "igemm_epilogue.h"

namespace PD_NS {

#define BLDS16(rsrc, ldsptr, voff, soff) \
  __builtin_amdgcn_raw_ptr_buffer_load_lds((rsrc), (__attribute__((address_space(3))) void*)(ldsptr), 16, (voff), (soff), 0, 0)
#define PD_OOB 0xffffff00u
#define VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define PHASE_SYNC()                   \
  __builtin_amdgcn_sched_barrier(0);   \
  __builtin_amdgcn_s_barrier();        \
  __builtin_amdgcn_sched_barrier(0)

namespace {
constexpr int FW = 16;                       // frame width = height: a 16-row MFMA tile is one image row, a 256-row tile one frame
constexpr int HW = FW + 2;                   // halo width
constexpr int HROWS = HW * HW;               // 324 halo rows
constexpr int PLROWS = 336;                  // rows allocated per plane: PLANE is a multiple of 256 B and 8 planes are whole 1 KB pieces
constexpr int PLANE = PLROWS * 16;
constexpr int HALO = 8 * PLANE;              // 43008 B
constexpr int NPIECE = HALO / 1024;          // 42
constexpr int WHT = 128 * 128;               // one W half tile: 128 rows x 128 B
constexpr int WBUF = 2 * WHT;
static_assert(PLANE % 256 == 0 && HALO % 1024 == 0 && PLROWS >= HROWS, "halo plane layout");
// level 1 (8 x 8 frames, four frame slots per tile): see "Level 1" in the header
constexpr int FW1 = 8;
constexpr int RP1 = 9;                       // row pitch: neighbouring image rows share their zero column
constexpr int FR1 = 81;                      // RP1 * RP1: a frame whose neighbour shares its zero row
constexpr int FPAIR1 = 88;                   // cells between the two frames of a wave row: 8 mod 16
constexpr int WROW1 = 169;                   // FPAIR1 + FR1: cells between the frame pairs of the two wave rows
constexpr int FREACH1 = 91;                  // cells a frame's fragment reads reach from its base: (FW1 + 1) * RP1 + FW1 + 2
constexpr int PLROWS1 = 352;
static_assert(FPAIR1 % 16 == 8 && FPAIR1 >= FR1 && WROW1 + FPAIR1 + FREACH1 <= PLROWS1, "level-1 halo plane layout");
constexpr int frame_base1(int f) { return (f >> 1) * WROW1 + (f & 1) * FPAIR1; }

template <int L>
struct Lay {                                 // L = 0: 16 x 16 frames, L = 1: 8 x 8 frames
  static constexpr int ROWS = L ? PLROWS1 : PLROWS;
  static constexpr int PLANE = ROWS * 16;
  static constexpr int HALO = 8 * PLANE;     // 43008 / 45056 B
  static constexpr int NPIECE = HALO / 1024; // 42 / 44
  static constexpr int NEXTRA = NPIECE - 40; // waves 0 .. NEXTRA - 1 issue a sixth piece
  static constexpr int PITCH = L ? RP1 : HW; // halo rows between two image rows
  static constexpr int W_OFF = 2 * HALO;
  static constexpr int LDS = W_OFF + 2 * WBUF;   // 151552 / 155648 B
  static_assert(PLANE % 256 == 0 && HALO % 1024 == 0 && NEXTRA >= 0 && NEXTRA <= 8, "halo plane layout");
  static_assert(LDS >= 8 * 128 * 32 * 4 && LDS <= 160 * 1024, "the epilogue stages 128 KB of accumulators in the operand buffers; a CU has 160 KB");
};

struct FragH {
  op8 v[2];
};
}  // namespace

template <int L, bool BORDER>
__global__ void __launch_bounds__(512) conv3d_halo_kernel(const pd_igemm_args p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int PLROWS = Lay<L>::ROWS, PLANE = Lay<L>::PLANE, HALO = Lay<L>::HALO, NEXTRA = Lay<L>::NEXTRA, PITCH = Lay<L>::PITCH,
                W_OFF = Lay<L>::W_OFF;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  // ---- XCD-aware tile id (bijective for any tile count) ----
  const int tiles_n = (p.N + 255) >> 8;
  const int tiles_m = L ? (p.M + 255) >> 8 : p.M >> 8;   // level 0: M = B * To * 256, whole tiles; level 1: M = B * To * 64
  const int nt = tiles_m * tiles_n;
  int t;
  {
    const int bid = blockIdx.x, xcd = bid & 7, q = nt >> 3, r = nt & 7;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int tm = t / tiles_n;                        // the tile's frame: sample * To + ot  (level 1: frames 4 tm .. 4 tm + 3)
  const int m0 = tm << 8;
  const int n0 = (t % tiles_n) << 8;

  const auto rA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, p.a_bytes, 0x00020000);
  const auto rW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, p.w_bytes, 0x00020000);

  // ---- W staging: one DMA instruction covers 64 rows x 128 B; thread -> (row tid/8, 16 B slot tid%8), swizzled source chunk ----
  const int srow = tid >> 3, spos = tid & 7;
  const uint32_t w_sel = (uint32_t)(spos ^ ((srow >> 1) & 7)) * 16u;
  uint32_t woff[2][2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = n0 + hh * 128 + i * 64 + srow;
      woff[hh][i] = n < p.N ? ((uint32_t)n * (uint32_t)p.ldw) * 2u + w_sel : PD_OOB;
    }
  // ---- halo staging: piece q = wave + 8 n covers cells [64 q, 64 q + 64) of the plane layout; this lane's cell -> (k-slot, halo row) ----
  uint32_t hoff[6];
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    const int cell = (wave + 8 * n) * 64 + lane;
    const int s = cell / PLROWS, r = cell - s * PLROWS;
    if constexpr (L == 0) {
      const int hr = r / HW, hc = r - hr * HW;
      const bool ok = cell < 8 * PLROWS && r < HROWS && hr >= 1 && hr <= FW && hc >= 1 && hc <= FW;
      hoff[n] = ok ? (uint32_t)((hr - 1) * FW + (hc - 1)) * (uint32_t)p.lda * 2u + (uint32_t)s * 16u : PD_OOB;
    } else {
      // level 1: source relative to the tile's first frame, with the cell's frame slot in bits 0-1 (the offset is a multiple of 16);
      // slot code 4 = never a pixel (zero row / column, pad and spare cells): no bit of the four-bit validity mask
      hoff[n] = PD_OOB | 4u;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int rel = r - frame_base1(f), hr = rel / RP1, hc = rel - hr * RP1;
        if (cell < 8 * PLROWS && rel >= 0 && rel < FR1 && hr >= 1 && hc >= 1)
          hoff[n] = ((uint32_t)(f * (FW1 * FW1) + (hr - 1) * FW1 + (hc - 1)) * (uint32_t)p.lda * 2u + (uint32_t)s * 16u) | (uint32_t)f;
      }
    }
  }

  // ---- groups: (channel chunk, kt), kt over the temporal taps whose input frame lies inside the sample ----
  const int kchunks = p.Cin >> 6;
  const int ot = tm % p.To;
  const bool dense = (p.debug_flags & 8) != 0;
  const int kt_lo = (dense || L) ? 0 : max(0, 1 - ot), kt_hi = (dense || L) ? 2 : min(2, p.Ti - ot);
  const int ngroups = (p.debug_flags & 1) ? 0 : kchunks * (kt_hi - kt_lo + 1);   // (bit 1: profiling, epilogue only)
  const uint32_t frame_b = (uint32_t)(L ? FW1 * FW1 : FW * FW) * (uint32_t)p.lda * 2u;   // bytes of one input frame
  // level 1: bit 4 kt + f = temporal tap kt of frame slot f reads a frame of the slot's own sample (and the slot is below M)
  uint32_t vm_all = 0;
  if constexpr (L == 1) {
    int o = (4 * tm) % p.To;
    for (int f = 0; f < 4; ++f) {
      if (4 * tm + f < p.B * p.To)
        for (int kt = 0; kt < 3; ++kt)
          if ((unsigned)(o - 1 + kt) < (unsigned)p.Ti) vm_all |= 1u << (4 * kt + f);
      if (++o == p.To) o = 0;
    }
  }
  const uint32_t w_tap_b = (uint32_t)p.w_tap_stride * 2u;

  // the halo stream runs one group ahead of the MFMAs, the W stream two K-tiles; all wave-uniform scalars
  int h_c = 0, h_kt = kt_lo, w_c = 0, w_kt = kt_lo;
  uint32_t w_off = (uint32_t)(kt_lo * 9) * w_tap_b;
  int h_soff = 0;
  uint32_t h_mask = 0, h_back = 0;
  char* const h_dst = smem + wave * 1024;            // + piece round * 8 KB + buffer * HALO  (lane * 16 is implicit)
  char* const w_dst = smem + W_OFF + wave * 1024;    // + half * WHT + i * (64 * 128) + buffer * WBUF
  auto next_halo = [&]() {                           // source of the halo stream's group, then advance the stream
    if constexpr (L == 0) {
      const int it = ot - 1 + h_kt;
      const bool ok = (unsigned)it < (unsigned)p.Ti;
      h_soff = __builtin_amdgcn_readfirstlane(ok ? (int)((uint32_t)(tm - 1 + h_kt) * frame_b + (uint32_t)h_c * 128u) : 0);
      h_mask = ok ? 0u : PD_OOB;
    } else {
      // slot f reads input frame 4 tm + f - 1 + kt; the scalar offset is never negative: in tile 0, kt = 0, it names frame 0 and the
      // lanes step one frame back (slot 0 is out of range there, so no lane that loads goes below the buffer)
      const int fin = 4 * tm - 1 + h_kt, fb = max(fin, 0);
      h_soff = __builtin_amdgcn_readfirstlane((int)((uint32_t)fb * frame_b + (uint32_t)h_c * 128u));
      h_back = (uint32_t)(fb - fin) * frame_b;
      h_mask = (vm_all >> (4 * h_kt)) & 15u;        // the four slots' validity
    }
    if (++h_kt > kt_hi) { h_kt = kt_lo; ++h_c; }
  };
  auto issue_h = [&](int n, int buf) {
    uint32_t v;
    if constexpr (L == 0) v = hoff[n] | h_mask;
    else v = ((h_mask >> (hoff[n] & 7u)) & 1u) ? (hoff[n] & ~7u) - h_back : PD_OOB;
    BLDS16(rA, h_dst + buf * HALO + n * 8192, v, h_soff);
  };
  auto next_w_group = [&]() {
    if (++w_kt > kt_hi) { w_kt = kt_lo; ++w_c; }
    w_off = (uint32_t)(w_kt * 9) * w_tap_b + (uint32_t)w_c * 128u;
  };
  auto issue_w = [&](int buf) {                      // both W halves of the W stream's K-tile, then the next tap of the group
    const int so = __builtin_amdgcn_readfirstlane((int)w_off);
    char* dst = w_dst + buf * WBUF;
    BLDS16(rW, dst, woff[0][0], so);
    BLDS16(rW, dst + 64 * 128, woff[0][1], so);
    BLDS16(rW, dst + WHT, woff[1][0], so);
    BLDS16(rW, dst + WHT + 64 * 128, woff[1][1], so);
    w_off += w_tap_b;
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  const int l16 = lane & 15, lg = lane >> 4;
  const int swz = (l16 >> 1) & 7;
  // + ((i + kh) * PITCH + kw) * 16 + ks * 4 * PLANE.  Level 1: MFMA row l16 of row tile i = pixel (i, l16 & 7) of frame slot 2 wr + (l16 >> 3)
  const int a_rd = (L ? wr * WROW1 + (l16 >> 3) * FPAIR1 + (l16 & 7) : wr * (8 * HW) + l16) * 16 + lg * PLANE;
  const int b_rd = W_OFF + (wc >> 1) * WHT + ((wc & 1) * 64 + l16) * 128;         // + tile * (16 * 128); slot ((ks*4 + lg) ^ swz)

  // ---- prologue: the halo of group 0, W of K-tiles 0 and 1 (a group has nine K-tiles: both exist) ----
  if (ngroups > 0) {
    next_halo();
    if (wave < NEXTRA) issue_h(5, 0);
#pragma unroll
    for (int n = 0; n < 5; ++n) issue_h(n, 0);
    issue_w(0);
    issue_w(1);
    VMCNT(4);
  }
  __builtin_amdgcn_s_barrier();
  if (wr == 1) __builtin_amdgcn_s_barrier();   // wave row 1 runs one barrier behind wave row 0
  __builtin_amdgcn_sched_barrier(0);

  FragH a[4], b0[2], b1[2];
#define LOAD_B(f, base) \
  (f).v[0] = *(const op8*)((base) + ((lg ^ swz) * 16)); (f).v[1] = *(const op8*)((base) + (((4 + lg) ^ swz) * 16))
#define LOAD_A(f, base) \
  (f).v[0] = *(const op8*)(base); (f).v[1] = *(const op8*)((base) + 4 * PLANE)
  // one quadrant: 4 row tiles x 2 column tiles x K = 64 (two k-steps); consecutive MFMAs hit different accumulators.  SK = local row tile
  // left out (-1: none): a[SK] is then neither loaded nor read, and six accumulators still lie between two MFMAs on the same one
#define QUAD16(R0, C0, bfrag, SK)                                                                           \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                          \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                           \
      if (i != (SK))                                                                                        \
        _Pragma("unroll") for (int c = 0; c < 2; ++c)                                                       \
          acc[(R0) + i][(C0) + c] = mfma_16x16x32(a[i].v[ks], bfrag[c].v[ks], acc[(R0) + i][(C0) + c]);

  int wcur = 0;
  // one group of nine K-tiles; has_next (another group follows: its halo and the W tiles of its first two K-tiles are issued here) is a
  // compile-time flag -- the last group is a second copy of the body, and the steady-state loop carries no test for it
  // WR: the wave row the copy is compiled for (border-row skip at level 0, where the all-zero row tiles differ between the wave rows: -1 = none)
  auto group = [&](auto has_next_t, auto wr_t, int g) {
    constexpr bool has_next = decltype(has_next_t)::value;
    constexpr int WR = decltype(wr_t)::value;
    constexpr bool skip_top = BORDER && (L == 1 || WR == 0), skip_bot = BORDER && (L == 1 || WR == 1);
    const int hnxt = (g & 1) ^ 1;
    const char* sA = smem + (g & 1) * HALO + a_rd;
    if (has_next) next_halo();
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int shift = ((j / 3) * PITCH + (j % 3)) * 16;    // byte offset of tap (kh, kw) inside a plane
      const char* sB = smem + wcur * WBUF + b_rd;
      const int skA = j < 3 && skip_top ? 0 : -1, skB = j >= 6 && skip_bot ? 3 : -1;   // local row tile left out: kh = j / 3, all compile-time
      // ---------- phase A: all four W column tiles, A row tiles 0-3; quadrants (A0, W0), (A0, W1); a halo piece of group g + 1 ----------
#pragma unroll
      for (int c = 0; c < 2; ++c) { LOAD_B(b0[c], sB + c * (16 * 128)); }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i != skA) { LOAD_A(a[i], sA + shift + i * (PITCH * 16)); }
#pragma unroll
      for (int c = 0; c < 2; ++c) { LOAD_B(b1[c], sB + (2 + c) * (16 * 128)); }
      if (j >= 1 && j <= 5 && has_next) {
        if (j == 1 && wave < NEXTRA) issue_h(5, hnxt);
        issue_h(j - 1, hnxt);
      }
      PHASE_SYNC();
      __builtin_amdgcn_s_setprio(1);
      QUAD16(0, 0, b0, skA)
      QUAD16(0, 2, b1, skA)
      __builtin_amdgcn_s_setprio(0);
      PHASE_SYNC();
      // ---------- phase B: A row tiles 4-7; quadrants (A1, W1), (A1, W0); W of K-tile k + 2; wait for K-tile k + 1 ----------
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i != skB) { LOAD_A(a[i], sA + shift + (4 + i) * (PITCH * 16)); }
      if (j <= 6 || has_next) {
        if (j == 7) next_w_group();
        issue_w(wcur);
        if (j >= 1 && j <= 5 && has_next) {
          VMCNT(5);                                          // this K-tile's halo piece and W pieces may still fly
        } else {
          VMCNT(4);
        }
      } else {
        VMCNT(0);
      }
      PHASE_SYNC();
      __builtin_amdgcn_s_setprio(1);
      QUAD16(4, 2, b1, skB)
      QUAD16(4, 0, b0, skB)
      __builtin_amdgcn_s_setprio(0);
      PHASE_SYNC();
      wcur ^= 1;
    }
  };
  auto groups = [&](auto wr_t) {
    for (int g = 0; g + 1 < ngroups; ++g) group(std::true_type{}, wr_t, g);
    if (ngroups > 0) group(std::false_type{}, wr_t, ngroups - 1);
  };
  if constexpr (L == 0 && BORDER) {            // one copy of the loop per wave row (wr is wave-uniform: a scalar branch, taken once)
    if (wr == 0) groups(std::integral_constant<int, 0>{});
    else groups(std::integral_constant<int, 1>{});
  } else {
    groups(std::integral_constant<int, -1>{});
  }
#undef QUAD16
#undef LOAD_A
#undef LOAD_B
  if (wr == 0) __builtin_amdgcn_s_barrier();   // re-join the two wave rows
  if (p.debug_flags & 2) return;               // (profiling: main loop only, nothing is stored)

  // ---- epilogue: two 32-column slabs per wave (8 waves x 128 x 32 fp32 = 128 KB of the operand buffers) ----
  float* sC = (float*)smem + wave * (128 * 32);
  const int m_base = m0 + wr * 128;
  const int m_end = min(p.M, m_base + 128);
  // accumulator register r of row tile i is MFMA row 4 lg + r; level 1: frame slot (4 lg + r) >> 3 of the wave row, pixel (i, (4 lg + r) & 7)
  const int c_row = L ? (lg >> 1) * 64 + (lg & 1) * 4 : 4 * lg;
  // (one call per slab, not a loop: a loop the unroller declines, the epilogue being long, would index acc[] at run time -- scratch)
  auto slab = [&](auto jsc) {
    constexpr int js = decltype(jsc)::value;
    // the slab aliases operand buffers that other waves may still read: one workgroup barrier; after it the slab is this wave's alone
    if (js == 0) __syncthreads();
    else igemm_epilogue_wave_sync();
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) sC[(c_row + i * (L ? 8 : 16) + r) * 32 + c * 16 + l16] = acc[i][js * 2 + c][r];
    igemm_epilogue_wave_sync();
    igemm_epilogue<128, 32>(p, sC, lane, m_base, m_end, n0 + wc * 64 + js * 32, 0);
  };
  slab(std::integral_constant<int, 0>{});
  slab(std::integral_constant<int, 1>{});
#endif
}

// true when the halo-staged kernel of this level can run the (already validated) launch: a one-product 16-bit 3x3x3, stride-1, pad-1,
// un-upsampled Conv3d on 16 x 16 frames (level 0; M = B * T * 256: every 256-row tile is one whole frame) or on 8 x 8 frames (level 1;
// M = B * T * 64: a tile is four frame slots, and a B * T that is no multiple of 4 is handled -- the slots past the last frame stage zeros
// and the epilogue stores no row >= M)
bool pd_conv3d_halo_supported(const pd_igemm_args& a, int kind, int level) {
  if (kind != 2 || a.split || a.fp8 || a.w_fold > 0 || a.nbatch > 1) return false;
  if (a.KT != 3 || a.KH != 3 || a.KW != 3 || a.pt != 1 || a.ph != 1 || a.pw != 1) return false;
  if (a.st != 1 || a.sh != 1 || a.sw != 1 || a.ut != 1 || a.uh != 1 || a.uw != 1 || a.vT > 0 || a.vH > 0 || a.vW > 0) return false;
  const int fw = level ? FW1 : FW;
  return a.Hi == fw && a.Wi == fw && a.Ho == fw && a.Wo == fw && a.Ti == a.To;
}

template <int L, bool BORDER>
static int launch_halo(const pd_igemm_args& a, hipStream_t s) {
  constexpr int LDS = Lay<L>::LDS;
  static bool attr_set_dev[PD_MAX_DEVICES];
  if (int rc = pd_raise_lds("pd_igemm", (const void*)conv3d_halo_kernel<L, BORDER>, LDS, attr_set_dev)) return rc;
  const int tiles = ((a.M + 255) / 256) * ((a.N + 255) / 256);
  hipLaunchKernelGGL((conv3d_halo_kernel<L, BORDER>), dim3(tiles, 1, 1), dim3(512), LDS, s, a);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

int pd_conv3d_halo_launch(const pd_igemm_args& a, int level, hipStream_t s) {
  if (a.debug_flags & 256) return level ? launch_halo<1, false>(a, s) : launch_halo<0, false>(a, s);   // (A/B: the dense MFMA schedule)
  return level ? launch_halo<1, true>(a, s) : launch_halo<0, true>(a, s);
}

}  // namespace PD_NS
