// attn_v6.h — attn_fwd_kernel6 / attn_fwd_causal_kernel6: the resident-K/V attention kernel for at most 128 keys (included by attn.hip, twice).
//
// v6 (Nkv <= 128: cross-attention over the 77 text tokens / 93 with image-prompt tokens / 16 IP tokens): v2's arithmetic, bit for
// bit, restructured for a launch that is bound by memory traffic and latency, not by the matrix pipe (two key tiles per query row).
//   * K and V^T of a (sample, head) are staged ONCE per workgroup and stay in LDS for a strip of `q_chunk` query rows: v2 staged
//     them per 128 rows — as many bytes from L2 as Q and O together — and paid their latency plus two block barriers per block;
//   * after that single barrier the four waves run independently over the strip's 128-row steps; the next step's Q rows are
//     requested before the current step computes;
//   * O leaves as whole 128-byte row segments: the normalised tile goes through 4 KB of wave-private LDS (16-byte chunk ^ (row & 7))
//     and is stored as 16 bytes per lane, 8 rows per instruction — v2 wrote 8 bytes per lane, 16 instructions per tile.
//
// This file is the kernel's text, included by attn.hip once per instance with ATTN6_KERNEL = its name and ATTN6_CAUSAL = false / true: two
// __global__ functions from one source.  (A shared __device__ body inlined into two kernels was tried first: hipcc then scheduled and allocated
// the non-causal instance differently — 1583 instructions for 1509 — while a second inclusion leaves it instruction for instruction as it was.)
//
// Causal form (attn_fwd_causal_kernel6, the CLIP text encoders' self-attention over 77 / 80 tokens): ATTN6_CAUSAL = true.
//   * key j is visible to query i iff j <= i and j < Nkv (top-left alignment; every row sees key 0, so no row is empty; rows >= Nkv - 1 see all keys);
//   * the mask (-1e30, like the key tail's) goes onto S' BEFORE the tile maximum: the reference maximum is taken over visible keys only, in the
//     t == 0 branch too.  A maximum that included a masked score far above the visible ones would push every visible probability to 2^-huge = 0
//     and the row to 0 / 0;
//   * a key tile whose first key lies above the last row of the wave's 32-row step is not computed at all, and a 16-key block above it gets no
//     exponentials and no P·V MFMAs — the wave-uniform branch of the padded blocks (q0 is an SGPR).  What is skipped were exact zeros: rows
//     below 64 take nothing from the second tile.
//   * a raise of the reference maximum is lane-local in effect: the branch is wave-uniform, but a row below the threshold gets d = 0.  The plain form
//     raises every row with a positive tile maximum once the wave branches; there a row's last bits may depend on its neighbours', which for a causal
//     row would be a dependence on future tokens.
// Every causal statement is behind a compile-time test of ATTN6_CAUSAL.
template <typename T>
__global__ __launch_bounds__(256, 2) void ATTN6_KERNEL(AttnP p, int q_chunk) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE + 4 * 4096];   // K[2], Vt[2], O staging per wave
  using V8 = typename Vec<T>::v8;
  using V4 = typename Vec<T>::v4;
  typedef T T2 __attribute__((ext_vector_type(2)));
  typedef float F2 __attribute__((ext_vector_type(2)));
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int h = blockIdx.y, b = blockIdx.z;
  const int bq = p.qk_src ? p.qk_src[b] : b;
  const int ntiles = (p.Nkv + KVB - 1) / KVB;       // 1 or 2

  {  // ---- K / V^T of the (sample, head): every tile, once
    const int srow = tid >> 3, schunk = tid & 7;
    const char* kbase = p.K + ((long)bq * p.k_bs + h * 64) * 2;
    const char* vbase = p.Vt + ((long)(b * p.heads + h) * 64) * (long)p.Nkv_pad * 2;
    for (int t = 0; t < ntiles; ++t) {
      const int kv0 = t * KVB;
#pragma unroll
      for (int ps = 0; ps < 2; ++ps) {
        const int row = ps * 32 + srow;
        const int key = kv0 + row;
        u32x4 z = {0u, 0u, 0u, 0u};
        const u32x4 hk = (key < p.Nkv) ? *(const u32x4*)(kbase + ((long)key * p.ldk + schunk * 8) * 2) : z;
        const u32x4 hv = *(const u32x4*)(vbase + ((long)row * p.Nkv_pad + kv0 + schunk * 8) * 2);
        const int off = row * 128 + ((schunk ^ ((row >> 1) & 7)) << 4);
        *(u32x4*)(smem + t * TILE + off) = hk;
        *(u32x4*)(smem + (2 + t) * TILE + off) = hv;
      }
    }
  }
  __syncthreads();

  const int q_begin = blockIdx.x * q_chunk;
  const int q_end = q_begin + q_chunk < p.Nq ? q_begin + q_chunk : p.Nq;
  char* ost = smem + 4 * TILE + w * 4096;
  auto load_q = [&](int q0, V8* raw) {
    int q = q0 + l31;
    if (q > p.Nq - 1) q = p.Nq - 1;
    const char* qp = p.Q + ((long)bq * p.q_bs + (long)q * p.ldq + h * 64) * 2;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) raw[ks] = *(const V8*)(qp + (ks * 16 + hi * 8) * 2);
  };
  V8 raw[4];
  int q0 = q_begin + w * 32;
  if (q0 < q_end) load_q(q0, raw);
  for (; q0 < q_end; q0 += QB) {
    V8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[ks][e] = (T)((float)raw[ks][e] * p.scale_log2e);
    if (q0 + QB < q_end) load_q(q0 + QB, raw);       // in flight under this step's MFMAs

    f32x16 o[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m_ref = 0.f, l_run = 0.f;
    f32x16 negm;
#pragma unroll
    for (int r = 0; r < 16; ++r) negm[r] = 0.f;

    for (int t = 0; t < ntiles; ++t) {
      const int kv0 = t * KVB;
      if constexpr (ATTN6_CAUSAL) {
        if (kv0 > q0 + 31) break;      // no row of this step sees a key of the tile (rows below 64, second tile)
      }
      const char* kt = smem + t * TILE;
      const char* vt = smem + (2 + t) * TILE;
      // ---- S' = K · Q'^T - m_ref
      f32x16 s[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = i * 32 + l31;
        s[i] = Vec<T>::mfma32(*(const V8*)(kt + row * 128 + ((hi ^ ((row >> 1) & 7)) << 4)), qf[0], negm);
      }
#pragma unroll
      for (int ks = 1; ks < 4; ++ks) {
        const int kc = ks * 2 + hi;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = i * 32 + l31;
          V8 kf = *(const V8*)(kt + row * 128 + ((kc ^ ((row >> 1) & 7)) << 4));
          s[i] = Vec<T>::mfma32(kf, qf[ks], s[i]);
        }
      }
      if constexpr (ATTN6_CAUSAL) {
        if (kv0 + KVB - 1 > q0 || kv0 + KVB > p.Nkv) {      // some row of the step has a masked key in this tile (uniform)
          const int last = q0 + l31 < p.Nkv - 1 ? q0 + l31 : p.Nkv - 1;      // the lane's row sees keys 0 .. last
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int key = kv0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
              if (key > last) s[i][r] = -1e30f;
            }
        }
      } else if (kv0 + KVB > p.Nkv) {      // key tail (last tile only)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kv0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (key >= p.Nkv) s[i][r] = -1e30f;
          }
      }
      // ---- tile maximum relative to the reference (pairs of fmaxf fuse into v_max3_f32)
      float mt = s[0][0];
#pragma unroll
      for (int r = 1; r < 16; r += 2) mt = fmaxf(fmaxf(mt, s[0][r]), r + 1 < 16 ? s[0][r + 1] : s[0][r]);
#pragma unroll
      for (int r = 0; r < 16; r += 2) mt = fmaxf(fmaxf(mt, s[1][r]), s[1][r + 1]);
      mt = fmaxf(mt, __shfl_xor(mt, 32));
      if (t == 0 || __builtin_amdgcn_ballot_w64(mt > ATTN_THR) != 0) {
        // raise (first tile: set) the reference: everything at the old reference is rescaled once, S' moves to the new one
        // causal: a row moves only when it is itself above the threshold (d = 0: alpha = 1, every update below is the identity), so that its bits
        // do not depend on whether a LATER row of the wave — a future token — triggered the branch
        const float d = t == 0 ? mt : ATTN6_CAUSAL ? (mt > ATTN_THR ? mt : 0.f) : fmaxf(mt, 0.f);
        const float alpha = t == 0 ? 1.f : __builtin_amdgcn_exp2f(-d);      // tile 0: O and l are still zero, and 2^-d is inf (0 * inf = NaN) where the row's first maximum is below -128
        m_ref += d;
        l_run *= alpha;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) { o[i][r] *= alpha; s[i][r] -= d; }
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[r] = -m_ref;
      }
      float psum = 0.f;
      // block (i, k2) = the tile's keys 16 (2 i + k2) .. + 15 = registers 8 k2 .. 8 k2 + 7 of s[i]: its probabilities, then O^T += V^T · P^T for it.
      // Round 6: a block without a real key is skipped.  77 text tokens are one whole tile + 13 keys of the second: 3 of its 4 blocks get no
      // exponentials, no conversions and no P·V MFMAs — 80 exponentials per lane and 32-row step instead of 128, in a loop that is bound by them.
      // A uniform branch (Nkv is a kernel argument); what is skipped were exact zeros (2^-1e30, 0 · V): the same output (a sum that is exactly -0
      // may come out +0).
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          if (kv0 + 16 * (2 * i + k2) >= p.Nkv) continue;      // no real key: its probabilities are exact zeros
          if constexpr (ATTN6_CAUSAL) {
            if (kv0 + 16 * (2 * i + k2) > q0 + 31) continue;   // above the step's last row: masked for every lane, exact zeros too
          }
          V8 pf;
#pragma unroll
          for (int r = 8 * k2; r < 8 * k2 + 8; r += 2) {
            const float e0 = __builtin_amdgcn_exp2f(s[i][r]);
            const float e1 = __builtin_amdgcn_exp2f(s[i][r + 1]);
            psum += e0 + e1;
            const T2 pk = __builtin_convertvector(F2{e0, e1}, T2);
            pf[r & 7] = pk[0];
            pf[(r & 7) + 1] = pk[1];
          }
          const int c0 = i * 4 + k2 * 2 + hi;
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) {
            const int row = dt * 32 + l31;
            const V8 vf = *(const V8*)(vt + row * 128 + ((c0 ^ ((row >> 1) & 7)) << 4));
            o[dt] = Vec<T>::mfma32(vf, pf, o[dt]);
          }
        }
      l_run += psum;
    }

    // ---- O: normalise, 16 bits, transpose through the wave's LDS strip, row-contiguous 16-byte stores
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = p.out_scale / l_tot;
    const int q = q0 + l31;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = o[dt][g * 4 + e] * inv;
        if (p.accumulate) {                          // the IP-Adapter branch adds into the text branch's output (same order as v2)
          if (q < p.Nq) {
            const V4 old = *(const V4*)(p.O + ((long)b * p.o_bs + (long)q * p.ldo + h * 64 + dt * 32 + 8 * g + 4 * hi) * 2);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += (float)old[e];
          }
        }
        V4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = (T)v[e];
        *(V4*)(ost + l31 * 128 + (((dt * 4 + g) ^ (l31 & 7)) << 4) + hi * 8) = out;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // one wave, in-order LDS: the tile is written before it is read back
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + (lane >> 3), ch = lane & 7;
      const u32x4 val = *(const u32x4*)(ost + row * 128 + ((ch ^ (row & 7)) << 4));
      const int qr = q0 + row;
      if (qr < p.Nq) *(u32x4*)(p.O + ((long)b * p.o_bs + (long)qr * p.ldo + h * 64 + ch * 8) * 2) = val;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // ... and read back before the next step overwrites it
  }
}
