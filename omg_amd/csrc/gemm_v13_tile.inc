// gemm_v13_tile.inc — the kernel of gemm_v13.h, included once per kernel NAME: gemm_kernel_v13 (OMG_V13_PH false) and gemm_phase_kernel_v13
// (true: a phase launch, GemmP in gemm_epilogue.h — the tap decode starts at (py - 1, px - 1) on the source image and the epilogue scatters
// rows to the phase's output pixels).  Two kernels from one text: every existing instantiation keeps its code and its name.
template <typename T, bool CONV, int EF>
__global__ __launch_bounds__(256, 1) void OMG_V13_KERNEL(GemmP p) {
  constexpr bool PH = OMG_V13_PH;
  static_assert(CONV || !PH, "PH is a form of the convolution");
  constexpr int MT = 4, NT = 5;
  constexpr int BM_ = MT * 64, BN_ = NT * 64, BKc = 64;
  constexpr int AB = MT * 2, WB = NT * 2;          // A / W row blocks (8 rows each) per wave per stage
  constexpr int NMM = MT * NT;                     // MFMAs per k-step
  constexpr int SLOTS = NMM / 2;                   // pairs of MFMAs per k-step
  constexpr int NRD = MT + NT;                     // fragment reads per k-step
  constexpr int A_BYTES = BM_ * BKc * 2;
  constexpr int STAGE_BYTES = (BM_ + BN_) * BKc * 2;
  static_assert(2 * STAGE_BYTES <= 160 * 1024, "two stages in LDS");

  const bool ts_on = (p.dbg & 16) && blockIdx.x < 8192 && threadIdx.x == 0;      // tools/gemm_timeline.py: per-block time stamps
  long long ts0 = 0, ts1 = 0, ts2 = 0;
  if (p.dbg & 16) ts0 = __builtin_amdgcn_s_memrealtime();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int l31 = lane & 31;

  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int tiles_per_group = p.tiles_m * p.tiles_n;
  const int grp = bid / tiles_per_group;
  const int t_in = bid - grp * tiles_per_group;
  int tm, tn;
  {
    const int per_group = 8 * p.tiles_n;
    const int gid = t_in / per_group;
    const int first_m = gid * 8;
    const int gsz = (p.tiles_m - first_m) < 8 ? (p.tiles_m - first_m) : 8;
    const int r = t_in - gid * per_group;
    tm = first_m + (r % gsz);
    tn = r / gsz;
  }
  const int m_base = (p.tile_groups > 1) ? grp * p.rows_per_group : 0;
  const int m_end = (p.tile_groups > 1) ? m_base + p.rows_per_group : p.M;
  const int m0 = m_base + tm * BM_;
  const int n0 = tn * BN_;
  int adapter = 0;
  if (p.group_adapter != nullptr) adapter = p.group_adapter[grp];
  if (p.w_adapter_stride != 0 && adapter < 0) return;
  const char* Wp = p.W + (p.w_adapter_stride != 0 ? (long)adapter * p.w_adapter_stride * 2 : 0);
  const int nk = (p.K + BKc - 1) / BKc;

  const int Ctot = p.C1 + p.C2;
  const long a_bytes = CONV ? (long)p.M / (p.Hout * p.Wout) * p.Hin * p.Win * p.C1 * 2 : ((long)(p.M - 1) * p.lda + p.K) * 2;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, (int)(a_bytes < 0x7fffff00 ? a_bytes : 0x7fffff00), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsA2 = __builtin_amdgcn_make_buffer_rsrc((void*)(CONV && p.X2 ? p.X2 : p.A), 0,
      CONV ? (int)((long)p.M / (p.Hout * p.Wout) * p.Hin * p.Win * p.C2 * 2) : 0, 0x00020000);
  const long w_bytes = ((long)(p.N - 1) * p.ldw + p.K) * 2;
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)Wp, 0, (int)w_bytes, 0x00020000);

  // DMA: one instruction moves 8 rows x 128 B; wave w owns row blocks w, w+4, ... of A (8 of 32) and of W (10 of 40)
  const int prow = lane >> 3, ppos = lane & 7;
  int voffA[AB], voffW[WB];
  int cb[AB], cy[AB], cx[AB];
  const int dchunk = (ppos ^ ((w & 1) * 4 + (prow >> 1))) * 16;   // ((row >> 1) & 7) with row = (w + 4i) * 8 + prow
#pragma unroll
  for (int i = 0; i < AB; ++i) {
    const int r = (w + i * 4) * 8 + prow;
    int gm = m0 + r; if (gm > m_end - 1) gm = m_end - 1;
    if constexpr (CONV) {
      const int hw = p.Hout * p.Wout;
      const int b = gm / hw; const int rem = gm - b * hw;
      cb[i] = b; cy[i] = rem / p.Wout; cx[i] = rem - cy[i] * p.Wout;
      voffA[i] = 0;
    } else {
      cb[i] = cy[i] = cx[i] = 0;
      voffA[i] = (int)((long)gm * p.lda * 2) + dchunk;
    }
  }
#pragma unroll
  for (int i = 0; i < WB; ++i) {
    const int r = (w + i * 4) * 8 + prow;
    int gn = n0 + r; if (gn > p.N - 1) gn = p.N - 1;
    voffW[i] = (int)((long)gn * p.ldw * 2) + dchunk;
  }
  const int ldo = w * 1024;

  const int wm = w >> 1, wn = w & 1;
  const int wn0 = n0 + wn * 128, wn4 = n0 + 256 + wn * 32;       // first column of the aligned group / of the odd block (header)
  f32x16 acc[MT][NT];
  using V8 = typename Vec<T>::v8;
  // A fragment i of k-step ks at aoff[ks] + i * 4096; W fragment j < 4 at boff[ks] + j * 4096 (tile rows 128 wn + 32 j), j = 4 at boff4[ks]
  // (tile rows 256 + 32 wn); every first row is a multiple of 32, so the swizzle term is the same
  int aoff[4], boff[4], boff4[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int sw = ((ks * 2 + hi) ^ ((l31 >> 1) & 7)) << 4;
    aoff[ks] = (wm * (MT * 32) + l31) * 128 + sw;
    boff[ks] = A_BYTES + (wn * 128 + l31) * 128 + sw;
    boff4[ks] = A_BYTES + (256 + wn * 32 + l31) * 128 + sw;
  }

  int koff = 0;
  int tap_dy = 0, tap_dx = 0, c0b = 0, xCb = 0;
  bool x2 = false;
  const int cpt = CONV ? Ctot / BKc : 1;
  const int pad = CONV ? (p.ksize == 3 ? 1 : 0) : 0;
  const int pad_y = PH ? 1 - (p.upsample >> 1) : pad, pad_x = PH ? 1 - (p.upsample & 1) : pad;
  const int ups = PH ? 0 : p.upsample;
  const int Hl = CONV ? (ups ? p.Hin * 2 : p.Hin) : 0;
  const int Wl = CONV ? (ups ? p.Win * 2 : p.Win) : 0;
#define OMG_PREP(kt_)                                                                                      \
  do {                                                                                                     \
    koff = (kt_) * (BKc * 2);                                                                              \
    if constexpr (CONV) {                                                                                  \
      const int tap = (kt_) / cpt; const int cc = (kt_) - tap * cpt;                                       \
      tap_dy = tap / p.ksize - pad_y; tap_dx = tap - (tap / p.ksize) * p.ksize - pad_x;                    \
      int c0 = cc * BKc;                                                                                   \
      x2 = c0 >= p.C1;                                                                                     \
      if (x2) c0 -= p.C1;                                                                                  \
      c0b = c0 * 2; xCb = (x2 ? p.C2 : p.C1) * 2;                                                          \
    }                                                                                                      \
  } while (0)
  // DMA instruction d of the prepared stage: d < AB -> A row block w + 4d, else W row block w + 4(d-AB); d < AB + WB
#define OMG_DMA(d_, nb_)                                                                                   \
  do {                                                                                                     \
    if ((d_) < AB) {                                                                                       \
      const int i_ = (d_) < AB ? (d_) : 0;                                                                 \
      if (CONV) dma16(x2 ? rsA2 : rsA, (nb_) + ldo + i_ * 4096,                                            \
                      conv_voff(cb[i_], cy[i_], cx[i_], dchunk, p.stride, tap_dy, tap_dx, Hl, Wl, ups, p.Hin, p.Win, xCb, c0b), 0); \
      else dma16(rsA, (nb_) + ldo + i_ * 4096, voffA[i_], koff);                                           \
    } else {                                                                                               \
      const int i_ = (d_) - AB < WB ? (d_) - AB : 0;                                                       \
      dma16(rsW, (nb_) + A_BYTES + ldo + i_ * 4096, voffW[i_], koff);                                      \
    }                                                                                                      \
  } while (0)
#define OMG_DMAN(first_, n_, nb_)                                                                          \
  do { _Pragma("unroll") for (int d_ = 0; d_ < (n_); ++d_) OMG_DMA((first_) + d_, nb_); } while (0)
#define OMG_WFRAG(sb_, ks_, j_) (*(const V8*)((sb_) + ((j_) < 4 ? boff[ks_] + (j_) * 4096 : boff4[ks_])))
#define OMG_RD(f_, sb_, ks_)                                                                               \
  do {                                                                                                     \
    _Pragma("unroll") for (int j = 0; j < NT; ++j) bf[f_][j] = OMG_WFRAG(sb_, ks_, j);                     \
    _Pragma("unroll") for (int i = 0; i < MT; ++i) af[f_][i] = *(const V8*)((sb_) + aoff[ks_] + i * 4096); \
  } while (0)
  // read order = order of first use by the MFMAs (n = NT i + j): W0, A0, W1 .. W4, A1 .. A3
#define OMG_RD1(f_, sb_, ks_, r_)                                                                          \
  do {                                                                                                     \
    const bool isA_ = (r_) == 1 || (r_) > NT;                                                              \
    const int idx_ = (r_) <= 1 ? 0 : (r_) <= NT ? (r_) - 1 : (r_) - NT;                                    \
    if (!isA_) bf[f_][idx_] = OMG_WFRAG(sb_, ks_, idx_);                                                   \
    else af[f_][idx_] = *(const V8*)((sb_) + aoff[ks_] + idx_ * 4096);                                     \
  } while (0)
  // acc[i][j] += W fragment j x A fragment i (the transposed tile), allocation class by j (header)
#define OMG_MM1(f_, n_)                                                                                    \
  do {                                                                                                     \
    if ((n_) % NT == 4) MfmaAsm<T>::v(acc[(n_) / NT][4], bf[f_][4], af[f_][(n_) / NT]);                    \
    else MfmaAsm<T>::a(acc[(n_) / NT][(n_) % NT], bf[f_][(n_) % NT], af[f_][(n_) / NT]);                   \
  } while (0)
  // slot s_ of a k-step: MFMA 2s, reads, MFMA 2s+1, DMAs.  RD_ = 1: one read per slot, 2: two per slot from the first slot on.
#define OMG_KSTEP(f_, RD_, rb_, rks_, DMA_, d0_, dn_, db_)                                                 \
  do {                                                                                                     \
    constexpr int RPS_ = (RD_) == 2 ? 2 : (NRD + SLOTS - 1) / SLOTS;                                       \
    constexpr int DPS_ = ((dn_) + SLOTS - 1) / SLOTS;                                                      \
    _Pragma("unroll") for (int s_ = 0; s_ < SLOTS; ++s_) {                                                 \
      OMG_MM1(f_, 2 * s_);                                                                                 \
      __builtin_amdgcn_sched_barrier(0);                                                                   \
      if ((RD_) != 0) {                                                                                    \
        _Pragma("unroll") for (int q_ = 0; q_ < RPS_; ++q_)                                                \
          if (s_ * RPS_ + q_ < NRD) OMG_RD1(1 - (f_), rb_, rks_, s_ * RPS_ + q_);                          \
      }                                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                   \
      OMG_MM1(f_, 2 * s_ + 1);                                                                             \
      __builtin_amdgcn_sched_barrier(0);                                                                   \
      if (DMA_) {                                                                                          \
        _Pragma("unroll") for (int q_ = 0; q_ < DPS_; ++q_)                                                \
          if (s_ * DPS_ + q_ < (dn_)) OMG_DMA((d0_) + s_ * DPS_ + q_, db_);                                \
      }                                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                   \
    }                                                                                                      \
  } while (0)

  V8 af[2][MT], bf[2][NT];
  // prologue: stage 0 completely, the A half of stage 1, the first fragments
  OMG_PREP(0);
  OMG_DMAN(0, AB + WB, smem);
  const bool gb_epi = acc_init_bias13<T>(p, acc, lane, m0, wn0, wn4);
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  if (p.dbg & 16) ts1 = __builtin_amdgcn_s_memrealtime();
  OMG_PREP(1);
  if (nk > 1) OMG_DMAN(0, AB, smem + STAGE_BYTES);
  OMG_RD(0, smem, 0);
  acc_fence(acc);            // the VALU writes of the initialisation are behind every MFMA's wait states

#define OMG_STAGE(HAS1_, HAS2_)                                                                            \
  do {                                                                                                     \
    const char* cur = smem + (kt & 1) * STAGE_BYTES;                                                       \
    char* nxt = smem + ((kt + 1) & 1) * STAGE_BYTES;                                                       \
    OMG_KSTEP(0, 1, cur, 1, HAS1_, AB, WB, nxt);                                                           \
    OMG_KSTEP(1, 1, cur, 2, false, 0, 0, nxt);                                                             \
    OMG_KSTEP(0, 1, cur, 3, false, 0, 0, nxt);                                                             \
    /* stage kt+1 has landed (this wave's part), this wave's reads of `cur` are complete: join the block */ \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier();              \
    if (HAS2_) OMG_PREP(kt + 2);                                                                           \
    OMG_KSTEP(1, (HAS1_) ? 2 : 0, nxt, 0, HAS2_, 0, AB, (char*)cur);                                       \
  } while (0)
  int kt = 0;
  for (; kt < nk - 2; ++kt) OMG_STAGE(true, true);
  if (kt < nk - 1) { OMG_STAGE(true, false); ++kt; }
  OMG_STAGE(false, false);
#undef OMG_STAGE
#undef OMG_PREP
#undef OMG_DMA
#undef OMG_DMAN
#undef OMG_WFRAG
#undef OMG_RD
#undef OMG_RD1
#undef OMG_MM1
#undef OMG_KSTEP
  acc_fence(acc);            // every MFMA has retired before anything reads an accumulator
  if (p.dbg & 32) {   // tools only: time the tile without its epilogue (the sum keeps the MFMAs alive)
    float sacc = 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc += acc[i][j][r];
    if (sacc == 1.2345e-30f) p.C[0] = 1;
    return;
  }
  if (p.dbg & 16) ts2 = __builtin_amdgcn_s_memrealtime();
  // XE: 8 KB per wave at the start of LDS — behind the last stage's barrier no wave reads a stage buffer any more (that stage issues no fragment
  // reads behind its barrier: its last k-step computes from registers)
  epilogue13<T, EF, PH>(p, acc, lane, m0 + wm * (MT * 32), wn0, wn4, m_end, gb_epi, smem + w * 8192);
  if (ts_on) {
    long long* t = omg_dbg_ts[blockIdx.x];
    t[0] = ts0; t[1] = ts1; t[2] = ts2; t[3] = __builtin_amdgcn_s_memrealtime();
    t[4] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));     // HW_REG_HW_ID, all 32 bits
    t[5] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));    // HW_REG_XCC_ID
  }
}
