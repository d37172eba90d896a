// gemm_tile128.inc — the 128x128x64 kernel of gemm.hip (v1), included once per kernel NAME: gemm_kernel (OMG_TILE128_PH false) and
// gemm_phase_kernel (true: a phase launch, GemmP in gemm_epilogue.h — tap origin (py - 1, px - 1) on the source image, rows scattered to the
// phase's output pixels).  Two kernels from one text, and not one template with a flag behind a wrapper: the wrapper alone moved the register
// counts of the existing instantiations, and the tests that count the conv kernels by name keep their numbers.
template <typename T, bool CONV, bool GLDS, bool CSEG = false>
__global__ __launch_bounds__(256, 2) void OMG_TILE128_KERNEL(GemmP p) {
  constexpr bool PH = OMG_TILE128_PH;
  static_assert(CONV || !CSEG, "CSEG is the segment of the CONV form; the plain form always has it");
  static_assert(!PH || (CONV && !CSEG), "PH is a form of the convolution without the segment");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int l31 = lane & 31;

  // ---- tile mapping: XCD-aware bijective remap, then M-fastest within the chunk
  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int tiles_per_group = p.tiles_m * p.tiles_n;
  const int grp = bid / tiles_per_group;
  const int t_in = bid - grp * tiles_per_group;
  // grouped ordering: 8 M-tiles x all N-tiles per group, M fastest inside the group, so that the ~32 consecutive
  // tiles an XCD receives touch ~8 A panels + <= 4..5 W panels instead of 32 + 1 (tall-skinny GEMMs re-read A per N tile)
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
  const int m0 = m_base + tm * BM;
  const int n0 = tn * BN;

  int adapter = 0;
  if (p.group_adapter != nullptr) adapter = p.group_adapter[grp];
  const bool seg2 = (p.K2 > 0) && (adapter >= 0);
  if (p.w_adapter_stride != 0 && adapter < 0) return;   // LoRA-down GEMM for a sample without adapter
  const char* Wp = p.W + (p.w_adapter_stride != 0 ? (long)adapter * p.w_adapter_stride * 2 : 0);
  const char* W2p = p.W2 + (seg2 ? (long)adapter * p.w2_adapter_stride * 2 : 0);
  const int a2off = (p.a2_col_block > 0) ? (n0 / p.a2_col_block) * p.K2 : 0;

  const int nk1 = (p.K + BK - 1) / BK;
  const int nk2 = seg2 ? (p.K2 + BK - 1) / BK : 0;
  const int nk = nk1 + nk2;

  // ---- per-lane staging coordinates: 4 A rows + 4 W rows per k-tile
  const int prow = lane >> 3;          // row within the 8-row DMA piece
  const int ppos = lane & 7;           // 16-B position within the 128-B row
  int arow[4];                         // global A row (clamped)
  int wrow[4];                         // global W row (clamped)
  int cb[4], cy[4], cx[4];             // conv: decoded output pixel
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = w * 32 + i * 8 + prow;
    int gm = m0 + r; if (gm > m_end - 1) gm = m_end - 1;
    int gn = n0 + r; if (gn > p.N - 1) gn = p.N - 1;
    arow[i] = gm; wrow[i] = gn;
    if constexpr (CONV) {
      const int hw = p.Hout * p.Wout;
      const int b = gm / hw; const int rem = gm - b * hw;
      cb[i] = b; cy[i] = rem / p.Wout; cx[i] = rem - cy[i] * p.Wout;
    }
  }
  const int Ctot = p.C1 + p.C2;
  const int cpt = CONV ? Ctot / BK : 1;   // k-tiles per tap
  const int pad = CONV ? (p.ksize == 3 ? 1 : 0) : 0;
  const char* zero = (const char*)omg_zero_page;

  u32x4 hold[8];
  char* ldsA = smem;
  char* ldsB = smem + 2 * TILE_BYTES;

  auto issue = [&](int kt, int buf) {
    const bool s2 = kt >= nk1;
    const int k0 = (s2 ? kt - nk1 : kt) * BK;
    const int Kseg = s2 ? p.K2 : p.K;
    // conv tap decode (wave-uniform)
    int dy = 0, dx = 0, c0 = k0;
    const char* xsrc = p.A; int xC = p.C1;
    if constexpr (CONV) {
      const int ktc = (CSEG && s2) ? 0 : kt;                   // a segment stage decodes no tap
      const int tap = ktc / cpt; const int cc = ktc - tap * cpt;
      dy = tap / p.ksize; dx = tap - dy * p.ksize;
      c0 = cc * BK;
      if (c0 >= p.C1) { xsrc = p.X2; xC = p.C2; c0 -= p.C1; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = w * 32 + i * 8 + prow;
      const int c = ppos ^ ((r >> 1) & 7);                    // source chunk for this LDS position
      const bool kvalid = (k0 + c * 8) < Kseg;
      // A operand
      const char* asrc;
      if constexpr (CONV) {
        int iy = cy[i] * p.stride + dy - (PH ? 1 - (p.upsample >> 1) : pad);
        int ix = cx[i] * p.stride + dx - (PH ? 1 - (p.upsample & 1) : pad);
        const int ups = PH ? 0 : p.upsample;
        const int Hl = ups ? p.Hin * 2 : p.Hin;
        const int Wl = ups ? p.Win * 2 : p.Win;
        const bool ok = (iy >= 0) && (iy < Hl) && (ix >= 0) && (ix < Wl);
        if (ups) { iy >>= 1; ix >>= 1; }
        const long pix = ((long)cb[i] * p.Hin + iy) * p.Win + ix;
        asrc = ok ? xsrc + (pix * xC + c0 + c * 8) * 2 : zero;
        if constexpr (CSEG) {
          if (s2) asrc = kvalid ? p.A2 + ((long)arow[i] * p.lda2 + k0 + c * 8) * 2 : zero;
        }
      } else {
        if (!s2) asrc = kvalid ? p.A + ((long)arow[i] * p.lda + k0 + c * 8) * 2 : zero;
        else     asrc = kvalid ? p.A2 + ((long)arow[i] * p.lda2 + a2off + k0 + c * 8) * 2 : zero;
      }
      stage16<GLDS>(asrc, ldsA + buf * TILE_BYTES + (w * 32 + i * 8) * 128, lane, hold[i]);
      // W operand
      const char* wsrc;
      if (!s2) wsrc = kvalid ? Wp + ((long)wrow[i] * p.ldw + (CONV ? kt * BK : k0) + c * 8) * 2 : zero;
      else     wsrc = kvalid ? W2p + ((long)wrow[i] * p.ldw2 + k0 + c * 8) * 2 : zero;
      stage16<GLDS>(wsrc, ldsB + buf * TILE_BYTES + (w * 32 + i * 8) * 128, lane, hold[4 + i]);
    }
  };
  auto commit = [&](int buf) {   // register-staged fallback: write the held chunks
    if constexpr (!GLDS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int off = (w * 32 + i * 8) * 128 + lane * 16;
        *(u32x4*)(ldsA + buf * TILE_BYTES + off) = hold[i];
        *(u32x4*)(ldsB + buf * TILE_BYTES + off) = hold[4 + i];
      }
    }
  };

  const int wm = w >> 1, wn = w & 1;
  f32x16 acc[2][2];
  acc_init_cols<T, 2, 2>(p, acc, lane & 31, n0 + wn * 64, m0);

  using V8 = typename Vec<T>::v8;

  issue(0, 0);
  commit(0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) issue(kt + 1, buf ^ 1);
    const char* a_base = ldsA + buf * TILE_BYTES;
    const char* b_base = ldsB + buf * TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      V8 af[2], bf[2];
      const int kc = ks * 2 + hi;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ra = wm * 64 + i * 32 + l31;
        af[i] = *(const V8*)(a_base + ra * 128 + ((kc ^ ((ra >> 1) & 7)) << 4));
        const int rb = wn * 64 + i * 32 + l31;
        bf[i] = *(const V8*)(b_base + rb * 128 + ((kc ^ ((rb >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = Vec<T>::mfma32(af[i], bf[j], acc[i][j]);
    }
    if constexpr (!GLDS) { if (kt + 1 < nk) commit(buf ^ 1); }
  }

  gemm_epilogue<T, PH>(p, acc, smem, w, lane, m0, n0, m_end);
}
