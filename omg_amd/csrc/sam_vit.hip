// sam_vit.hip — what SAM's ViT image encoder (omg_amd/sam_vit.py) needs beside omg_gemm, omg_layernorm and omg_conv3x3_nhwc_act, for gfx950.
//
//   omg_attn_relpos   softmax attention per head with SAM's decomposed relative-position bias, straight from the fused QKV projection:
//                       score(q, k) = scale q.k + q.Rh[qy - ky + Sh - 1] + q.Rw[qx - kx + Sw - 1]        (the bias terms on the UNSCALED q)
//                     global (window == 0: every token of the sample is a key) and windowed (window == S: the S x S window of the query,
//                     positions beyond the H x W grid being real keys with k | v = pad_kv).  Flash style: neither the scores nor the bias
//                     ever leave the chip, and the windows are indexed in place (no partition / unpartition pass, no padded buffer).
//   omg_gelu_erf      the MLP's activation (omg_gemm has no plain GELU epilogue): the erf form through gelu.h.
//
// attn_relpos_kernel.  A window is the unit: a KH x KW key grid at origin (oy, ox) of the token grid (global mode: ONE window, the grid
// itself).  A workgroup = 4 waves = 128 consecutive queries of a window (row-major inside the window), a wave = 32 of them; every
// workgroup walks all key tiles (64 keys) of its window.  The structure is attn_v7.h's: swapped products S^T = K Q^T (keys on the
// accumulator registers, the query on the lane) and O^T = V^T P^T, so that P goes from the accumulator into the next MFMA's B operand
// without leaving the registers, and V^T fragments come out of the row-major V tile by ds_read_b64_tr_b16.  What differs:
//   * head_dim 64 | 80: D / 16 k-steps, ceil(D / 32) row blocks of O^T (the third block of 80 is half used); LDS rows of 2 D + 16 bytes
//     (36 / 44 banks: sixteen consecutive rows start on sixteen different 16-byte slots, so the b128 fragment reads are conflict-free
//     without a swizzle);
//   * K / V tiles are staged through registers, not by LDS-DMA: the source of a row is a token of the grid, the pad row or nothing, and the
//     loads of tile t + 1 are in flight under the MFMAs of tile t;
//   * the bias.  Once per query block two small products  R . Q^T  (the table rows on the registers, the query on the lane) give, per
//     query, q.Rh[j] and q.Rw[j] for every j; each lane scatters what it holds into the wave's own LDS table as  bh[ky] = q.Rh[qy - ky
//     + KH - 1]  and  bw[kx]  (fp32, already in the exp2 domain), index-major so that the 32 lanes of a half hit 32 banks.  In the
//     tile loop the fp32 score of key (ky, kx) becomes  fma(q.k, scale log2e, bh[ky] + bw[kx] - m)  BEFORE the tile maximum.
//     ROW64 form (global mode, W == 64 — SAM's 64 x 64 grid): a key tile is exactly one image row, so bw is the same 32 registers for
//     every tile (read once) and bh one LDS read per tile; the table then holds bh only.
// Softmax: fp32, exp2 domain, a reference maximum that is raised when a tile exceeds it by more than 2^RP_THR (attn_v7.h's scheme),
// the row sum in fp32 on the unrounded probabilities, one rounding at the store.
#include "common.h"

namespace {

constexpr int RP_KVB = 64;                 // keys per tile
constexpr float RP_LOG2E = 1.4426950408889634f;
constexpr float RP_THR = 8.0f;             // probabilities stay below 2^8 relative to the reference maximum
constexpr float RP_MASKED = -1e30f;

template <typename T> struct RpTrRead;
template <> struct RpTrRead<f16> {
  typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 raw4;
  static OMG_DEV f16x4 rd(const char* lds) {
    return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) raw4*)lds));
  }
};
template <> struct RpTrRead<bf16> {
  typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 raw4;
  static OMG_DEV bf16x4 rd(const char* lds) {
    return __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) raw4*)lds));
  }
};

struct RelposP {
  const char* qkv; long ld;              // [B H W][ld] elements: q | k | v, each heads * D wide
  char* out; long ldo;                   // [B H W][ldo]
  const char* Rh; const char* Rw;        // [2 KH - 1][D], [2 KW - 1][D]
  const char* pad_kv;                    // [2 heads D]: k | v of a position beyond the grid, or null (zeros)
  int heads, H, W;
  int KH, KW;                            // the key grid of a window
  int nwx, nqb;                          // windows per row of windows; 128-query blocks per window
  int tabn;                              // floats per query in a wave's bias table
  float scale_log2e;
};

// n / d for 0 <= n < 2^22, 1 <= d: the float estimate is within one of the quotient, the remainder test settles it
OMG_DEV void rp_divmod(int n, int d, float inv_d, int& q, int& r) {
  q = (int)(((float)n + 0.5f) * inv_d);
  r = n - q * d;
  if (r < 0) { q -= 1; r += d; }
  else if (r >= d) { q += 1; r -= d; }
}

// accumulator register r of lane half hi -> row of the 32-row MFMA result
OMG_DEV int rp_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

template <typename T, int D, bool ROW64>
__global__ __launch_bounds__(256, 2) void attn_relpos_kernel(RelposP p) {
  constexpr int CH = D / 8;                        // 16-byte chunks per row
  constexpr int KS = D / 16;                       // k-steps of the score product
  constexpr int DT = (D + 31) / 32;                // 32-row blocks of O^T
  constexpr int STRIDE = D * 2 + 16;               // LDS row, bytes
  constexpr int TILE_B = RP_KVB * STRIDE + 64;     // + what the transposing reads of the last, half-used d block run past the last row
  constexpr int NIT = 2 * RP_KVB * CH / 256;       // staging chunks per lane: 4 | 5
  extern __shared__ __attribute__((aligned(16))) char rp_smem[];
  using V8 = typename Vec<T>::v8;
  using V4 = typename Vec<T>::v4;
  typedef T T2 __attribute__((ext_vector_type(2)));
  typedef float F2 __attribute__((ext_vector_type(2)));
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int h = blockIdx.y, b = blockIdx.z;
  const int win = blockIdx.x / p.nqb, qb = blockIdx.x - win * p.nqb;
  const int wy = win / p.nwx, wx = win - wy * p.nwx;
  const int oy = wy * p.KH, ox = wx * p.KW;
  const int KH = p.KH, KW = p.KW, NK = KH * KW;
  const int ntiles = (NK + RP_KVB - 1) / RP_KVB;
  const float inv_kw = 1.0f / (float)KW;
  char* kt = rp_smem;
  char* vt = rp_smem + TILE_B;
  float* tab = (float*)(rp_smem + 2 * TILE_B) + (long)w * 32 * p.tabn;
  const long hd = (long)p.heads * D;               // width of q, of k and of v
  const char* base = p.qkv + (long)b * p.H * p.W * p.ld * 2;

  // ---- the lane's query: index qi inside the window -> (qy, qx) there -> token (oy + qy, ox + qx).  A query beyond the window or beyond
  // the grid is computed as a copy of the window's first one (always inside the grid) and never stored.
  int qi = qb * 128 + w * 32 + l31, qy, qx;
  bool valid = qi < NK;
  rp_divmod(valid ? qi : 0, KW, inv_kw, qy, qx);
  valid = valid && oy + qy < p.H && ox + qx < p.W;
  if (!valid) { qy = 0; qx = 0; }
  const long qtok = (long)(oy + qy) * p.W + (ox + qx);
  const bool active = __builtin_amdgcn_ballot_w64(valid) != 0;      // wave-uniform: a wave without a query only helps staging

  // ---- staging through registers: the K tile and the V tile are 2 * 64 * CH = NIT * 256 chunks of 16 bytes, lane -> chunks it * 256 + tid
  u32x4 sreg[NIT];
  auto load_tile = [&](const int t) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int c2 = it * 256 + tid;
      const int isv = c2 >= RP_KVB * CH ? 1 : 0;
      const int c = c2 - isv * RP_KVB * CH;
      const int row = c / CH, ch = c - row * CH;
      u32x4 z = {0u, 0u, 0u, 0u};
      const int key = t * RP_KVB + row;
      if (key < NK) {
        int ky, kx;
        if constexpr (ROW64) { ky = t; kx = row; }
        else rp_divmod(key, KW, inv_kw, ky, kx);
        const int y = oy + ky, x = ox + kx;
        if (y < p.H && x < p.W) z = *(const u32x4*)(base + (((long)y * p.W + x) * p.ld + (1 + isv) * hd + (long)h * D + ch * 8) * 2);
        else if (p.pad_kv != nullptr) z = *(const u32x4*)(p.pad_kv + (isv * hd + (long)h * D + ch * 8) * 2);
      }
      sreg[it] = z;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int c2 = it * 256 + tid;
      const int isv = c2 >= RP_KVB * CH ? 1 : 0;
      const int c = c2 - isv * RP_KVB * CH;
      const int row = c / CH, ch = c - row * CH;
      *(u32x4*)(kt + isv * TILE_B + row * STRIDE + ch * 16) = sreg[it];
    }
  };
  load_tile(0);

  // ---- Q fragments (B operand: column = query l31, k = 8 hi + e of k-step ks), unscaled
  V8 qf[KS];
  {
    const char* qp = base + (qtok * p.ld + (long)h * D) * 2;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const V8*)(qp + (ks * 16 + hi * 8) * 2);
  }

  // ---- bias tables of the wave's 32 queries.  R . Q^T: register r of the j-group g is row j = 32 g + rp_row(r, hi) of R for the lane's
  // query; it is the bias of key coordinate kc = qc + S - 1 - j.  dst[kc * 32 + l31], kc in [0, S).
  auto build_table = [&](const char* R, const int S, const int qc, float* dst) {
    const int nrows = 2 * S - 1;
    for (int g = 0; g * 32 < nrows; ++g) {
      int j = g * 32 + l31;
      if (j > nrows - 1) j = nrows - 1;
      const char* rp = R + ((long)j * D + hi * 8) * 2;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = Vec<T>::mfma32(*(const V8*)(rp + ks * 32), qf[ks], acc);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kc = qc + S - 1 - (g * 32 + rp_row(r, hi));
        if (kc >= 0 && kc < S) dst[kc * 32 + l31] = acc[r] * RP_LOG2E;
      }
    }
  };
  float bw[2][16];
  if (active) {
    if constexpr (ROW64) {
      build_table(p.Rw, KW, qx, tab);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // one wave, in-order LDS: the table is written before it is read back
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) bw[i][r] = tab[(i * 32 + rp_row(r, hi)) * 32 + l31];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // ... and read before bh overwrites it
      build_table(p.Rh, KH, qy, tab);
    } else {
      build_table(p.Rh, KH, qy, tab);
      build_table(p.Rw, KW, qx, tab + KH * 32);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }

  // transposing reads of the V tile (attn_v7.h): a group of 16 lanes fetches a [4 keys][16 d] block, lane i16 supplies the address of d
  // 4 (i16 & 3) .. + 3 of key (i16 >> 2) and receives the four keys of d = i16.  Group g = lane >> 4: d block 16 (g & 1), keys 4 hi + 0..3
  // (read 0) and 8 + 4 hi + 0..3 (read 1) of a 16-key group — the key order of the P registers.
  int vtr[2];
  {
    const int i16 = lane & 15, g1 = (lane >> 4) & 1;
#pragma unroll
    for (int r = 0; r < 2; ++r) vtr[r] = (8 * r + 4 * hi + (i16 >> 2)) * STRIDE + (16 * g1 + 4 * (i16 & 3)) * 2;
  }

  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m_ref = 0.f, l_run = 0.f;

  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();                                   // nobody reads tile t - 1 any more
    store_tile();
    __syncthreads();
    if (t + 1 < ntiles) load_tile(t + 1);              // in flight under this tile's MFMAs
    if (!active) continue;
    const int kv0 = t * RP_KVB;

    // A half tile (32 keys) at a time — its own maximum test, its own probabilities — so that 16 score registers are live, not 32.
    float bh = 0.f;
    if constexpr (ROW64) bh = tab[t * 32 + l31];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k0 = kv0 + i * 32;
      if (k0 >= NK) continue;                            // no key at all (wave-uniform)
      // ---- S^T = K . Q^T (raw dot products)
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
      const char* kr = kt + (i * 32 + l31) * STRIDE + hi * 16;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s = Vec<T>::mfma32(*(const V8*)(kr + ks * 32), qf[ks], s);
      // ---- exp2 domain, bias, relative to the reference maximum
      if constexpr (ROW64) {
        const float bhm = bh - m_ref;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = __builtin_fmaf(s[r], p.scale_log2e, bw[i][r] + bhm);
      } else {
        const float* tabw = tab + KH * 32;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          int ky, kx;
          rp_divmod(k0 + 8 * g + 4 * hi, KW, inv_kw, ky, kx);                  // the first of four consecutive keys
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kyc = ky < KH - 1 ? ky : KH - 1;                         // keys past the window (masked below) read a valid entry
            const float bias = tab[kyc * 32 + l31] + tabw[kx * 32 + l31];
            s[g * 4 + e] = __builtin_fmaf(s[g * 4 + e], p.scale_log2e, bias - m_ref);
            kx += 1;
            if (kx == KW) { kx = 0; ky += 1; }
          }
        }
      }
      if (k0 + 32 > NK) {                                // key tail (wave-uniform); key k0 itself is real
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (k0 + rp_row(r, hi) >= NK) s[r] = RP_MASKED;
      }
      float mt = s[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s[r]);
      mt = fmaxf(mt, __shfl_xor(mt, 32));
      const bool first = t == 0 && i == 0;
      if (first || __builtin_amdgcn_ballot_w64(mt > RP_THR) != 0) {
        // raise (first keys: set) the reference: what was summed at the old one is rescaled once
        const float d = first ? mt : fmaxf(mt, 0.f);
        const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-d);
        m_ref += d;
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] -= d;
      }
      // ---- P = 2^S', O^T += V^T . P^T per group of 16 keys (registers 8 k2 .. 8 k2 + 7); a group without a key is skipped
      float psum = 0.f;
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        if (k0 + 16 * k2 >= NK) continue;
        V8 pf;
#pragma unroll
        for (int r = 8 * k2; r < 8 * k2 + 8; r += 2) {
          const float e0 = __builtin_amdgcn_exp2f(s[r]);
          const float e1 = __builtin_amdgcn_exp2f(s[r + 1]);
          psum += e0 + e1;
          const T2 pk = __builtin_convertvector(F2{e0, e1}, T2);
          pf[r & 7] = pk[0];
          pf[(r & 7) + 1] = pk[1];
        }
        const char* vg = vt + (32 * i + 16 * k2) * STRIDE;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const V4 lo = RpTrRead<T>::rd(vg + vtr[0] + dt * 64);
          const V4 hi4 = RpTrRead<T>::rd(vg + vtr[1] + dt * 64);
          const V8 vf = __builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
          o[dt] = Vec<T>::mfma32(vf, pf, o[dt]);
        }
      }
      l_run += psum;
    }
  }

  // ---- O: the lane holds four consecutive d of its query per (d block, register group): d = 32 dt + 8 g + 4 hi + 0..3
  if (!active) return;
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.0f / l_tot;
  if (!valid) return;
  char* op = p.out + (((long)b * p.H * p.W + qtok) * p.ldo + (long)h * D) * 2;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = dt * 32 + 8 * g + 4 * hi;
      if (d0 < D) {                                  // D = 80: groups 2, 3 of the third block do not exist
        V4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = (T)(o[dt][g * 4 + e] * inv);
        *(V4*)(op + d0 * 2) = out;
      }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void gelu_erf_kernel(const char* X, char* Y, long nvec) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  float x[8];
  load8<T>(X + i * 16, x);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = gelu_f(x[e]);
  store8<T>(Y + i * 16, x);
}

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

template <typename T, int D, bool ROW64>
int relpos_launch(const RelposP& p, dim3 grid, size_t lds, hipStream_t s) {
  OMG_LAUNCH((attn_relpos_kernel<T, D, ROW64>), grid, dim3(256), lds, s, p);
  return omg_check_launch("attn_relpos");
}

}  // namespace

extern "C" int omg_attn_relpos(int dtype, int B, int H, int W, int heads, int head_dim, int window, const void* qkv, int64_t ld,
                               const void* rel_h, const void* rel_w, const void* pad_kv, float scale, void* out, int64_t ldo, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_attn_relpos: dtype");
  OMG_REQUIRE(head_dim == 64 || head_dim == 80, "omg_attn_relpos: head_dim 64 or 80");
  OMG_REQUIRE(B >= 0 && H >= 0 && W >= 0 && heads >= 1, "omg_attn_relpos: B, H, W >= 0, heads >= 1");
  OMG_REQUIRE(window >= 0 && (long)window * window <= 256, "omg_attn_relpos: window 0 (global) or S with S * S <= 256");
  if (B == 0 || H == 0 || W == 0) return OMG_OK;
  OMG_REQUIRE(qkv && rel_h && rel_w && out, "omg_attn_relpos: null operand");
  OMG_REQUIRE(H <= 4096 && W <= 4096 && (long)H * W <= (1L << 22), "omg_attn_relpos: H, W at most 4096 and H * W at most 2^22");
  OMG_REQUIRE(B <= 65535 && heads <= 65535, "omg_attn_relpos: grid limits");
  const int64_t hd = (int64_t)heads * head_dim;
  OMG_REQUIRE(ld >= 3 * hd && ldo >= hd, "omg_attn_relpos: row stride below 3 heads head_dim (qkv) / heads head_dim (out)");
  OMG_REQUIRE(ld % 8 == 0 && ldo % 8 == 0, "omg_attn_relpos: row strides multiples of 8");
  OMG_REQUIRE(aligned16(qkv) && aligned16(rel_h) && aligned16(rel_w) && aligned16(pad_kv) && aligned16(out), "omg_attn_relpos: 16-byte aligned operands");
  RelposP p;
  p.qkv = (const char*)qkv; p.ld = (long)ld;
  p.out = (char*)out; p.ldo = (long)ldo;
  p.Rh = (const char*)rel_h; p.Rw = (const char*)rel_w; p.pad_kv = (const char*)pad_kv;
  p.heads = heads; p.H = H; p.W = W;
  p.KH = window ? window : H;
  p.KW = window ? window : W;
  p.nwx = window ? (W + window - 1) / window : 1;
  const long nwin = window ? (long)p.nwx * ((H + window - 1) / window) : 1;
  p.nqb = (p.KH * p.KW + 127) / 128;
  const bool row64 = window == 0 && W == 64;
  p.tabn = row64 ? (H > 64 ? H : 64) : p.KH + p.KW;
  p.scale_log2e = scale * RP_LOG2E;
  const size_t lds = 2 * (size_t)(RP_KVB * (head_dim * 2 + 16) + 64) + (size_t)4 * 32 * p.tabn * sizeof(float);
  OMG_REQUIRE(lds <= 64 * 1024, "omg_attn_relpos: bias tables beyond 64 KB of LDS (global mode: H + W <= 83, or W == 64 and H <= 335)");
  OMG_REQUIRE(nwin * p.nqb <= 0x7fffffffL, "omg_attn_relpos: grid limits");
  const dim3 grid((unsigned)(nwin * p.nqb), (unsigned)heads, (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
#define OMG_RP(T_, D_) return row64 ? relpos_launch<T_, D_, true>(p, grid, lds, s) : relpos_launch<T_, D_, false>(p, grid, lds, s)
  if (dtype == OMG_F16) { if (head_dim == 64) OMG_RP(f16, 64); else OMG_RP(f16, 80); }
  if (head_dim == 64) OMG_RP(bf16, 64); else OMG_RP(bf16, 80);
#undef OMG_RP
}

extern "C" int omg_gelu_erf(int dtype, const void* X, void* Y, int64_t n, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_gelu_erf: dtype");
  OMG_REQUIRE(X && Y, "omg_gelu_erf: null operand");
  OMG_REQUIRE(n >= 0 && n % 8 == 0, "omg_gelu_erf: n a multiple of 8");
  OMG_REQUIRE(aligned16(X) && aligned16(Y), "omg_gelu_erf: 16-byte aligned operands");
  if (n == 0) return OMG_OK;
  const long nvec = n / 8;
  OMG_REQUIRE((nvec + 255) / 256 <= 0x7fffffffL, "omg_gelu_erf: grid limits");
  const dim3 grid((unsigned)((nvec + 255) / 256));
  if (dtype == OMG_F16) OMG_LAUNCH(gelu_erf_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)X, (char*)Y, nvec);
  else OMG_LAUNCH(gelu_erf_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)X, (char*)Y, nvec);
  return omg_check_launch("gelu_erf");
}
