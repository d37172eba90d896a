// gemm_v13.h — the product kernel of the 256 x 320 x 64 tile (variant 28), FOUR waves (2 x 2 waves of 128 x 160 — 20 accumulator tiles = 320
// registers per lane).  Written in round 4, first run and landed in round 5 (profiles/r05_exp_v13_*.log: bitwise equal with every other variant;
// +15 ... 17 % on the N = 320 / 640 convolutions against the 128 x 320 tile, +3 ... 23 % on the 256-tile convolutions, +8 ... 18 % on the
// N = 640 / 1920 Linears, behind the 256 x 256 ring kernel where N = 1280 fills whole rounds of both; the whole benchmark +3.1 %).
//
// Why this tile:
//   * 320 = the width unit of the SDXL UNet (320 / 640 / 960 / 1280 / 1920 / 2560 / 3840): every N of the workload except the GEGLU projection is a whole
//     number of 320-wide tiles, where the 256-wide tile pads N = 640 to 768 (+20 % work) and N = 320 / 640 convolutions run the 128 x 320 tile of v7
//     (0.7 fragment reads per MFMA, 56 KB of LDS-DMA per 5.2 MFLOP);
//   * per MFMA it needs LESS of everything the 256 x 256 tile is short of: 0.45 fragment reads (256^2: 0.5), 72 KB of LDS-DMA per 10.5 MFLOP (64 KB per
//     8.4), 11 % fewer operand bytes from L2 per FLOP — and 25 % more work behind every tile's 7 - 9 us of prologue + epilogue + dispatch gap.
// Round 1 tried this tile as gemm_kernel_v7<.., 4, 5> and dropped it: with the MFMA builtin hipcc keeps all 320 accumulators in one allocation class
// and moves 1000 - 1300 of them between the AGPR and the VGPR half EVERY STAGE, plus 500 bytes of scratch (the same instantiation, compiled again in
// round 4: 1280 v_accvgpr_* + 88 scratch accesses in the steady-state stage).  Here the MFMAs are inline asm with the allocation class of each accumulator
// written in the constraint — acc[i][0..3] "+a" (256 AGPRs), acc[i][4] "+v" (64 VGPRs) — and the steady-state stage of the Linear kernel is 80 MFMAs,
// 36 ds_read_b128, 18 LDS-DMA, 11 VALU, no accumulator move, no scratch (tests/test_codeobj.py checks that on every EXP build).
// What inline-asm MFMAs cost: the hazard recogniser does not see them.  Nothing but MFMAs touches an accumulator between the two fences below
// (acc_fence: an asm that names all 20 accumulators and carries the wait states), so the only hazards are VALU write -> first MFMA (fence in front of
// the loop) and last MFMA -> first epilogue read (fence behind it; without it hipcc hoisted v_accvgpr_read one instruction behind the MFMA that
// produces the value).
//
// K loop: gemm_kernel_v7's (two 72 KB stages, fragments one k-step ahead in two register sets, one barrier per stage in front of its last k-step,
// the W half of stage kt + 1 issued over k-step 0 and the A half of stage kt + 2 over k-step 3, one LDS-DMA per two MFMAs).  The five-buffer ring of
// gemm_v11.h does not fit: 3 x 32 KB + 2 x 40 KB = 176 KB.
// Column ownership: wave column wn owns the 128 columns [128 wn, 128 wn + 128) (j = 0..3) and the 32 columns [256 + 32 wn, + 32) (j = 4), so that
// both waves' 128-column groups start on a 256-byte boundary of the output row: XE (variant 28) sends them through the transposed streaming epilogue
// of gemm_epilogue.h unchanged (whole 256-byte row segments, nt) and stores the odd 32 columns register-direct without nt (the two waves' halves of that
// 128-byte line meet in L2).  (Storing everything register-direct, as the 128 x 320 tile does — variant 27 of the experiment — was 1 ... 12 % slower.)
// Epilogue forms: 1 bias only, 4 per-row group bias / SiLU / residual decided per unit, 5 residual by register-direct loads.  No GEGLU (a 160-wide wave
// tile cannot hold whole [32 value | 32 gate] blocks): the launcher returns such problems to the 256 x 256 kernel.
// Values: the same loads, the same MFMA order per accumulator, the same epilogue arithmetic as every other variant — bitwise identical by construction.
// This header is included inside gemm.hip's anonymous namespace.

template <typename T> struct MfmaAsm;
template <> struct MfmaAsm<f16> {
  static OMG_DEV void a(f32x16& c, f16x8 x, f16x8 y) { asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(x), "v"(y)); }
  static OMG_DEV void v(f32x16& c, f16x8 x, f16x8 y) { asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(c) : "v"(x), "v"(y)); }
};
template <> struct MfmaAsm<bf16> {
  static OMG_DEV void a(f32x16& c, bf16x8 x, bf16x8 y) { asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(x), "v"(y)); }
  static OMG_DEV void v(f32x16& c, bf16x8 x, bf16x8 y) { asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(x), "v"(y)); }
};
// All 20 accumulators pass through these four statements (an asm takes at most 30 operands; "+" counts twice): whatever reads or writes an
// accumulator on the other side is ordered against every MFMA, and the first statement carries the wait states (s_nop 15 = 16 of them; a 16-pass
// MFMA result needs 18 before a VALU / v_accvgpr read — the MFMAs in front of the last one have long retired, the pipe is in order).
OMG_DEV void acc_fence(f32x16 (&acc)[4][5]) {
  asm volatile("s_nop 15\n\ts_nop 15" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[0][2]), "+a"(acc[0][3]), "+v"(acc[0][4]));
  asm volatile("" : "+a"(acc[1][0]), "+a"(acc[1][1]), "+a"(acc[1][2]), "+a"(acc[1][3]), "+v"(acc[1][4]));
  asm volatile("" : "+a"(acc[2][0]), "+a"(acc[2][1]), "+a"(acc[2][2]), "+a"(acc[2][3]), "+v"(acc[2][4]));
  asm volatile("" : "+a"(acc[3][0]), "+a"(acc[3][1]), "+a"(acc[3][2]), "+a"(acc[3][3]), "+v"(acc[3][4]));
}

// first output column of column block j of the wave: j < 4 -> the aligned 128-column group, j = 4 -> the odd 32 columns
#define OMG_V13_COL(j_, wn0_, wn4_) ((j_) < 4 ? (wn0_) + (j_) * 32 : (wn4_))

// acc_init_bias (gemm_epilogue.h) for the column ownership above: accumulators start at bias (+ the folded per-sample bias)
template <typename T>
OMG_DEV bool acc_init_bias13(const GemmP& p, f32x16 (&acc)[4][5], int lane, int m0, int wn0, int wn4) {
  const int hi = lane >> 5;
  const bool fold_gb = fold_group_bias(p);
  const __amdgpu_buffer_rsrc_t rsB = epi_rsrc(p.bias, (long)p.N * 2);
  const __amdgpu_buffer_rsrc_t rsG = epi_rsrc(fold_gb ? p.group_bias + (long)(m0 / p.rows_per_group) * p.ldgb * 2 : nullptr, (long)p.N * 2);
  u32x4 rb[5][2], rg[5][2];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const int c = OMG_V13_COL(j, wn0, wn4) + pr * 16 + hi * 8;      // c >= N is beyond num_records: zeros
      rb[j][pr] = __builtin_amdgcn_raw_buffer_load_b128(rsB, c * 2, 0, 0);
      rg[j][pr] = __builtin_amdgcn_raw_buffer_load_b128(rsG, c * 2, 0, 0);
    }
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      float f[8], g[8];
      decode_runs<T>(rb[j][pr], f);
      decode_runs<T>(rg[j][pr], g);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][j][pr * 8 + e] = f[e] + g[e];
    }
  return p.group_bias != nullptr && !fold_gb;
}

// epilogue_rows (gemm_epilogue.h) for the 128 x 160 wave tile.  RS / GENERIC as there; the units of j < 4 go through xe_put / xe_flush (the
// EpiCtx<4> view cx4 is all those two read), the units of j = 4 are stored register-direct.  Same arithmetic, same packing, same bits.
template <typename T, bool RS, bool GENERIC, bool PH = false>
OMG_DEV void epilogue_rows13(const GemmP& p, f32x16 (&acc)[4][5], const EpiCtx<5>& cx, const EpiCtx<4>& cx4, int lane_col4, bool has_gb) {
  const float osc = p.out_scale;
  const bool has_rs = GENERIC ? p.residual != nullptr : RS;
  u32x4 rraw[2][5][2];          // residual of row block i: the lane's 10 16-byte units, fetched one row block ahead
#define OMG_V13_LCOL(j_) ((j_) < 4 ? cx.lane_col : lane_col4)
#define OMG_V13_SOFF(j_, pr_) ((((j_) < 4 ? (j_) * 32 : 0) + (pr_) * 16) * 2)
#define OMG_FETCH_RES13(i_, buf_)                                                                          \
  do {                                                                                                     \
    const int gm_ = cx.wm0 + (i_) * 32 + cx.l31;                                                           \
    const int rrow_ = gm_ < cx.m_end ? gm_ * (int)p.ldr * 2 : EPI_OOB;                                     \
    _Pragma("unroll") for (int j = 0; j < 5; ++j)                                                          \
      _Pragma("unroll") for (int pr = 0; pr < 2; ++pr)                                                     \
        rraw[buf_][j][pr] = __builtin_amdgcn_raw_buffer_load_b128(cx.rsR, (rrow_ + OMG_V13_LCOL(j)) | cx.voob[j][pr], OMG_V13_SOFF(j, pr), 0); \
  } while (0)
  if (has_rs) OMG_FETCH_RES13(0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gm = cx.wm0 + i * 32 + cx.l31;
    const bool row_ok = gm < cx.m_end;
    if (has_rs && i + 1 < 4) OMG_FETCH_RES13(i + 1, (i + 1) & 1);
    int orow = gm;
    if constexpr (PH) orow = phase_out_row(p, gm);
    const int crow = row_ok ? orow * (int)p.ldc * 2 : EPI_OOB;
    const int grow = GENERIC && has_gb && row_ok ? ((gm / p.rows_per_group) * (int)p.ldgb) * 2 : EPI_OOB;
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = acc[i][j][pr * 8 + e];
        if constexpr (GENERIC) {
          if (has_gb) {
            float f[8];
            load_runs<T>(cx.rsG, (grow + OMG_V13_LCOL(j)) | cx.voob[j][pr], OMG_V13_SOFF(j, pr), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += f[e];
          }
          if (p.act == OMG_ACT_SILU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = silu_fast(v[e]);
          }
        }
        if (has_rs) {
          const u32x4 rr = rraw[i & 1][j][pr];
          unsigned q[4] = {rr[0], rr[1], rr[2], rr[3]};
          swap_runs<T>(q);
          u32x4 sw = {q[0], q[1], q[2], q[3]};
          float rf[8];
          unpack8<T>(sw, rf);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf(v[e], osc, rf[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] *= osc;
        }
        if (j < 4) xe_put<T, 256>(cx4, 4 * j + 2 * pr, v);
        else store_runs<T>(cx.rsC, (crow + OMG_V13_LCOL(j)) | cx.voob[j][pr], OMG_V13_SOFF(j, pr), v);
        __builtin_amdgcn_sched_barrier(0);
      }
    xe_flush<T, 256, PH>(p, cx4, i, cx4.wn0);
  }
#undef OMG_FETCH_RES13
#undef OMG_V13_SOFF
#undef OMG_V13_LCOL
}

template <typename T, int EF, bool PH = false>
OMG_DEV void epilogue13(const GemmP& p, f32x16 (&acc)[4][5], int lane, int wm0, int wn0, int wn4, int m_end, bool has_gb, char* xl) {
  static_assert(EF == 1 || EF == 4 || EF == 5, "forms of the 256 x 320 tile: bias only, generic, residual");
  EpiCtx<5> cx;
  cx.hi = lane >> 5; cx.l31 = lane & 31; cx.wm0 = wm0; cx.m_end = m_end;
  if constexpr (PH) cx.rsC = epi_rsrc(p.C, ((4L * p.M - 1) * p.ldc + p.N) * 2);      // a phase launch scatters its M rows over the 4 M rows of the output
  else cx.rsC = epi_rsrc(p.C, ((long)(p.M - 1) * p.ldc + p.N) * 2);
  cx.rsR = epi_rsrc(p.residual, ((long)(p.M - 1) * p.ldr + p.N) * 2);
  cx.rsG = epi_rsrc(has_gb ? p.group_bias : nullptr, EPI_CLAMP);
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) cx.voob[j][pr] = (OMG_V13_COL(j, wn0, wn4) + pr * 16 + cx.hi * 8 < p.N && !(p.dbg & 1024)) ? 0 : EPI_OOB;
  cx.lane_col = (wn0 + cx.hi * 8) * 2;
  cx.wn0 = wn0; cx.n_out = p.N; cx.xl = xl; cx.rl = nullptr;
  const int lane_col4 = (wn4 + cx.hi * 8) * 2;
  EpiCtx<4> cx4;                 // what xe_put / xe_flush read
  cx4.rsC = cx.rsC; cx4.rsR = cx.rsR; cx4.rsG = cx.rsG;
  cx4.hi = cx.hi; cx4.l31 = cx.l31; cx4.wm0 = wm0; cx4.m_end = m_end; cx4.lane_col = cx.lane_col; cx4.wn0 = wn0; cx4.n_out = p.N; cx4.xl = xl; cx4.rl = nullptr;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) cx4.voob[j][pr] = cx.voob[j][pr];
  if constexpr (EF == 1) epilogue_rows13<T, false, false, PH>(p, acc, cx, cx4, lane_col4, false);
  else if constexpr (EF == 5) epilogue_rows13<T, true, false, PH>(p, acc, cx, cx4, lane_col4, false);
  else epilogue_rows13<T, false, true, PH>(p, acc, cx, cx4, lane_col4, has_gb);
}

// The kernel's text is gemm_v13_tile.inc, compiled under two names: gemm_kernel_v13 and gemm_phase_kernel_v13 (phase launches, CONV only).
#define OMG_V13_KERNEL gemm_kernel_v13
#define OMG_V13_PH false
#include "gemm_v13_tile.inc"
#undef OMG_V13_KERNEL
#undef OMG_V13_PH
#define OMG_V13_KERNEL gemm_phase_kernel_v13
#define OMG_V13_PH true
#include "gemm_v13_tile.inc"
#undef OMG_V13_KERNEL
#undef OMG_V13_PH
#undef OMG_V13_COL

template <typename T, bool CONV, int EF, bool PH = false>
int launch_v13(GemmP p, hipStream_t s, int mrows) {
  constexpr int lds = 2 * (256 + 320) * 64 * 2;
  static bool attr = false;
  if (!attr) {
    attr = true;
    if constexpr (PH) (void)hipFuncSetAttribute((const void*)gemm_phase_kernel_v13<T, true, EF>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    else (void)hipFuncSetAttribute((const void*)gemm_kernel_v13<T, CONV, EF>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  }
  p.tiles_m = (mrows + 255) / 256;
  p.tiles_n = (p.N + 319) / 320;
  p.dbg = g_dbg;
  const int grid = p.tile_groups * p.tiles_m * p.tiles_n;
  if (grid <= 0) return OMG_OK;
  if constexpr (PH) {
    OMG_LAUNCH((gemm_phase_kernel_v13<T, true, EF>), dim3(grid), dim3(256), lds, s, p);
  } else {
    OMG_LAUNCH((gemm_kernel_v13<T, CONV, EF>), dim3(grid), dim3(256), lds, s, p);
  }
  return omg_check_launch("gemm_v13");
}
// GEGLU problems are not this tile's (header): the caller sends them to the 256 x 256 kernel
template <typename T, bool CONV>
int launch_v13_form(const GemmP& p, hipStream_t s, int mrows) {
  const bool gb_rows = p.group_bias != nullptr && p.rows_per_group % 256 != 0;       // == !fold_group_bias
  if (gb_rows || p.act == OMG_ACT_SILU) return launch_v13<T, CONV, 4>(p, s, mrows);
  if (p.residual != nullptr) return launch_v13<T, CONV, 5>(p, s, mrows);
  return launch_v13<T, CONV, 1>(p, s, mrows);
}
// phase launches: no residual (refused by the host), so the bias-only and the generic form
template <typename T>
int launch_v13_phase(const GemmP& p, hipStream_t s, int mrows) {
  const bool gb_rows = p.group_bias != nullptr && p.rows_per_group % 256 != 0;
  if (gb_rows || p.act == OMG_ACT_SILU) return launch_v13<T, true, 4, true>(p, s, mrows);
  return launch_v13<T, true, 1, true>(p, s, mrows);
}
