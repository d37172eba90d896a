// gdino.hip — what GroundingDINO's feature enhancer (omg_amd/gdino.py: transformers' GroundingDinoEncoder and the neck in front of it)
// needs beside omg_gemm, omg_layernorm, omg_groupnorm_res_act, omg_conv3x3_nhwc_act, omg_relu and omg_add_inplace, for gfx950.
//
//   omg_msdeform_attn     multi-scale deformable attention between its Linear layers: the softmax over the L P logits, the sampling
//                         locations, the bilinear taps (align_corners = False, zero padding) and their weighted sum, one launch.
//   omg_attn_bi_vision    the image side of GroundingDinoBiMultiHeadAttention (head_dim 256): softmax over the T text keys, times the
//                         text values, per image row.
//   omg_attn_bi_text      its text side: softmax over ALL N image keys, times the image values, per text token — the keys split into
//                         chunks across workgroups, fp32 partials (maximum, sum, accumulator) in the workspace, a second launch folds
//                         them in chunk order.
//   omg_attn_masked       softmax attention at head_dim 64 under a byte mask [B, Nq, Nk] (the text enhancer's self-attention).
// and, for the decoder behind it (omg_amd/gdino_decoder.py; its other kernels are in gdino_decoder.hip), the same two bodies again:
//   omg_msdeform_attn_box msdeform_body with BOX reference points [B, Nq, L, 4] (cx, cy, w, h).
//   omg_attn_hd32         attn_tiled_body at head_dim 32 under a key mask [B, Nk]: any Nq, Nk.
// A body is a device function and every entry a kernel of its own name (msdeform_kernel / msdeform_box_kernel, attn_tiled_kernel /
// attn_hd32_kernel), so the enhancer's kernels are the instances they were.
//
// msdeform_kernel.  FOUR lanes are one (query, head): lane `sub` owns channels 8 sub .. 8 sub + 7 of the head's 32, so a tap is one
// 16-byte load per lane and the four lanes read one 64-byte row piece.  Every lane forms the softmax and the locations of its (query,
// head) itself (the loads of the four lanes are the same addresses); per level the 4 points x 4 corners = 16 row pieces are loaded
// before the first is used.  The sum runs level by level, point by point, corners (y0 x0), (y0 x1), (y1 x0), (y1 x1), in fp32 with
// one rounding at the store.  A corner beyond the level, or on a masked value row, has weight 0 and is read from a clamped address.
//
// attn_tiled_kernel<D, MASK2D, PARTIAL>.  The three attention entries are one kernel.  A workgroup is 64 query rows (a wave owns 16) of
// one (sample, head) against the keys [kbeg, kend) in LDS tiles of 64: K rows [64][D] and V TRANSPOSED [D][64].
//   scores    S^T = K Q^T, v_mfma_f32_16x16x32 over D / 32 steps per 16-key tile, the lane holding for its query (lane & 15) the keys
//             4 (lane >> 4) + r of every key tile;
//   softmax   fp32, exp2 domain, the scale folded into the exponent (scale log2 e) on the fp32 score; an excluded key (mask, tile
//             padding) is -1e30; online over the 64-key tiles: running maximum m, sum l and accumulator rescaled by 2^(m - m');
//   P V       O^T = V^T P^T by v_mfma_f32_16x16x16, whose B operand is the score layout: P is rounded to 16 bits in registers; the
//             sum l is taken on the ROUNDED probabilities (numerator and denominator see the same P);
//   store     O / l rounded once (PARTIAL = false), or m, l and the unnormalised accumulator in fp32 (PARTIAL = true), which
//             attn_fold_kernel combines over the chunks in ascending order: M = max m_c, O = sum_c 2^(m_c - M) O_c / sum_c 2^(m_c - M) l_c.
// Every reduction has a fixed order that depends on the sample's own sizes only: a result depends neither on the batch nor on the launch.
#include "common.h"

namespace {

constexpr float GD_LOG2E = 1.4426950408889634f;
constexpr float GD_EXCLUDED = -1e30f;

template <typename T> struct GdMfma;
template <> struct GdMfma<f16> {
  static OMG_DEV f32x4 k16(f16x4 a, f16x4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
};
template <> struct GdMfma<bf16> {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  static OMG_DEV f32x4 k16(bf16x4 a, bf16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
  }
};

// ------------------------------------------------------------------ multi-scale deformable attention
struct MsdP {
  const char* value; long ldv;           // [B N][ldv]
  const unsigned char* mask;             // [B N], 0: the row reads as zeros; or null
  const char* ow; long ldow;             // [B Nq][ldow]: offsets (head, level, point, xy) | logits (head, level point)
  const float* ref;                      // [B Nq L 2] (x, y); BOX: [B Nq L 4] (cx, cy, w, h)
  char* out; long ldo;                   // [B Nq][ldo]
  int N, Nq, heads;
  long pairs;                            // B Nq heads
  int H[4], W[4], start[4];
};

template <typename T, int L, bool MASK, bool BOX>
OMG_DEV void msdeform_body(const MsdP& p) {
  constexpr int P = 4;
  using V4 = typename Vec<T>::v4;
  const int sub = threadIdx.x & 3;
  const long pair = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  if (pair >= p.pairs) return;
  const long row = pair / p.heads;                 // b Nq + q
  const int h = (int)(pair - row * p.heads);
  const long b = row / p.Nq;
  const char* owr = p.ow + row * p.ldow * 2;

  // ---- softmax over the L P logits: the maximum and the sum here, a level's four weights again where the level is sampled
  const char* lgp = owr + ((long)p.heads * L * P * 2 + (long)h * L * P) * 2;
  float mx = GD_EXCLUDED;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const V4 lg = *(const V4*)(lgp + l * P * 2);
#pragma unroll
    for (int i = 0; i < P; ++i) mx = fmaxf(mx, (float)lg[i] * GD_LOG2E);
  }
  float sum = 0.f;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const V4 lg = *(const V4*)(lgp + l * P * 2);
#pragma unroll
    for (int i = 0; i < P; ++i) sum += __builtin_amdgcn_exp2f((float)lg[i] * GD_LOG2E - mx);
  }
  const float inv = 1.0f / sum;

  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  const char* vbase = p.value + ((long)h * 32 + sub * 8) * 2;
  // a loop, not unrolled: one level's 16 row pieces are in flight, not all L levels' (64 registers instead of 256)
#pragma unroll 1
  for (int l = 0; l < L; ++l) {
    const int Hl = p.H[l], Wl = p.W[l];
    const long r0 = b * p.N + p.start[l];
    float off[8];
    load8<T>(owr + ((long)h * L * P * 2 + l * P * 2) * 2, off);
    const V4 lg = *(const V4*)(lgp + l * P * 2);
    float rx, ry, sx = 0.f, sy = 0.f;
    if (BOX) {
      // box reference (cx, cy, w, h): loc = c + off / 4 * (w, h) * 0.5, pixel x = cx W + off_x (w W / 8) - 0.5.  The step per unit of
      // offset, s = w (W / 8), is ONE rounding (W / 8 is exact); the coordinate is fma(cx, W, fma(off, s, -0.5)): two more.
      const f32x4 r4 = *(const f32x4*)(p.ref + (row * L + l) * 4);
      rx = r4[0]; ry = r4[1];
      sx = r4[2] * ((float)Wl * 0.125f); sy = r4[3] * ((float)Hl * 0.125f);
    } else {
      rx = p.ref[(row * L + l) * 2]; ry = p.ref[(row * L + l) * 2 + 1];
    }
    u32x4 raw[P * 4];
    float wt[P * 4];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      // pixel coordinate of loc = ref + off / (W, H) under align_corners = False: loc W - 0.5.  Beyond [-2, n + 1] every corner is
      // outside whatever the value, so the clamp changes no result and keeps the conversion to int defined (a NaN takes the bound).
      float x = __builtin_fmaf(rx, (float)Wl, BOX ? __builtin_fmaf(off[2 * i], sx, -0.5f) : off[2 * i] - 0.5f);
      float y = __builtin_fmaf(ry, (float)Hl, BOX ? __builtin_fmaf(off[2 * i + 1], sy, -0.5f) : off[2 * i + 1] - 0.5f);
      x = fminf(fmaxf(x, -2.0f), (float)Wl + 1.0f);
      y = fminf(fmaxf(y, -2.0f), (float)Hl + 1.0f);
      const float xf = floorf(x), yf = floorf(y);
      const float lx = x - xf, ly = y - yf;
      const int x0 = (int)xf, y0 = (int)yf;
      const float a = __builtin_amdgcn_exp2f((float)lg[i] * GD_LOG2E - mx) * inv;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int xx = x0 + (c & 1), yy = y0 + (c >> 1);
        const bool in = xx >= 0 && xx < Wl && yy >= 0 && yy < Hl;
        const int xc = min(max(xx, 0), Wl - 1), yc = min(max(yy, 0), Hl - 1);
        const long vr = r0 + (long)yc * Wl + xc;
        float w = ((c & 1) ? lx : 1.0f - lx) * ((c >> 1) ? ly : 1.0f - ly) * a;
        bool keep = in;
        if (MASK) keep = keep && p.mask[vr] != 0;
        wt[i * 4 + c] = keep ? w : 0.f;
        raw[i * 4 + c] = *(const u32x4*)(vbase + vr * p.ldv * 2);
      }
    }
#pragma unroll
    for (int t = 0; t < P * 4; ++t) {
      float f[8];
      unpack8<T>(raw[t], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(wt[t], f[e], acc[e]);
    }
  }
  store8<T>(p.out + (row * p.ldo + (long)h * 32 + sub * 8) * 2, acc);
}

// the two entries are kernels of their own names: point references [B Nq L 2] and box references [B Nq L 4]
template <typename T, int L, bool MASK>
__global__ __launch_bounds__(256) void msdeform_kernel(MsdP p) { msdeform_body<T, L, MASK, false>(p); }
template <typename T, int L, bool MASK>
__global__ __launch_bounds__(256) void msdeform_box_kernel(MsdP p) { msdeform_body<T, L, MASK, true>(p); }

// ------------------------------------------------------------------ tiled attention
struct AtP {
  const char *q, *k, *v;                 // rows of ld* elements, samples q/k/v_bs elements apart; head h at column h D
  long ldq, q_bs, ldk, k_bs, ldv, v_bs;
  const unsigned char* mask;             // MASK2D: [B Nq Nk], else [B Nk]; 1 = attend; or null
  char* out; long ldo, o_bs;             // PARTIAL = false
  float* ws;                             // PARTIAL = true: [B heads nchunks] x (acc [Nq][D] | m [Nq] | l [Nq])
  int heads, Nq, Nk, chunk, nchunks;
  float scale_log2e;
};

template <typename T, int D, bool MASK2D, bool PARTIAL>
OMG_DEV void attn_tiled_body(const AtP& p) {
  constexpr int KT = 64;                       // keys per LDS tile
  constexpr int KSTR = D * 2 + 16;             // K row, bytes: sixteen consecutive rows start on different 16-byte slots
  constexpr int VSTR = KT * 2 + 16;            // V^T row, bytes
  constexpr int CH = D / 8;                    // 16-byte chunks per row
  using V8 = typename Vec<T>::v8;
  using V4 = typename Vec<T>::v4;
  __shared__ __attribute__((aligned(16))) char kt[KT * KSTR];
  __shared__ __attribute__((aligned(16))) char vt[D * VSTR];
  __shared__ unsigned char km[KT];             // !MASK2D: 1 = the tile's key takes part
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, l15 = lane & 15;
  const int h = blockIdx.y % p.heads, c = blockIdx.y / p.heads, b = blockIdx.z;
  const int q0 = blockIdx.x * 64 + w * 16;
  const bool active = q0 < p.Nq;               // wave-uniform: a wave without rows only helps to stage
  const int qi = q0 + l15;
  const bool qvalid = qi < p.Nq;
  const int kbeg = c * p.chunk, kend = min(p.Nk, kbeg + p.chunk);
  const char* kb = p.k + ((long)b * p.k_bs + (long)h * D) * 2;
  const char* vb = p.v + ((long)b * p.v_bs + (long)h * D) * 2;

  // ---- the lane's query: a row beyond Nq is computed as a copy of the last row and never stored
  V8 qf[D / 32];
  if (active) {
    const char* qp = p.q + ((long)b * p.q_bs + (long)(qvalid ? qi : p.Nq - 1) * p.ldq + (long)h * D + g * 8) * 2;
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) qf[kk] = *(const V8*)(qp + kk * 64);
  }
  float m = GD_EXCLUDED, lsum = 0.f;
  f32x4 o[D / 16];
#pragma unroll
  for (int db = 0; db < D / 16; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = kbeg; k0 < kend; k0 += KT) {
    const int nk = min(KT, kend - k0);
    const int nt = (nk + 15) >> 4;             // 16-key tiles of this LDS tile
    __syncthreads();
    // ---- K rows: chunk = (key i, 8 channels ch); rows nk .. 16 nt - 1 are zeros
    for (int cc = tid; cc < nt * 16 * CH; cc += 256) {
      const int i = cc / CH, ch = cc - i * CH;
      u32x4 kz = {0u, 0u, 0u, 0u};
      if (i < nk) kz = *(const u32x4*)(kb + ((long)(k0 + i) * p.ldk + ch * 8) * 2);
      *(u32x4*)(kt + i * KSTR + ch * 16) = kz;
    }
    // ---- V^T: a wave's lanes are 64 keys of one chunk column, so its 2-byte stores fill rows of V^T contiguously
    for (int cc = tid; cc < KT * CH; cc += 256) {
      const int i = cc & 63, ch = cc >> 6;
      if (i >= nt * 16) continue;
      u32x4 vz = {0u, 0u, 0u, 0u};
      if (i < nk) vz = *(const u32x4*)(vb + ((long)(k0 + i) * p.ldv + ch * 8) * 2);
      const V8 v8 = __builtin_bit_cast(V8, vz);
#pragma unroll
      for (int e = 0; e < 8; ++e) *(T*)(vt + (ch * 8 + e) * VSTR + i * 2) = v8[e];
    }
    if (!MASK2D && tid < KT)
      km[tid] = (tid < nk && (p.mask == nullptr || p.mask[(long)b * p.Nk + k0 + tid] != 0)) ? 1 : 0;
    __syncthreads();
    if (!active) continue;

    // ---- S^T = K . Q^T per key tile; register r of tile t is key 16 t + 4 g + r
    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < nt) {
#pragma unroll
        for (int kk = 0; kk < D / 32; ++kk) {
          const V8 kf = *(const V8*)(kt + (t * 16 + l15) * KSTR + kk * 64 + g * 16);
          s[t] = Vec<T>::mfma16(kf, qf[kk], s[t]);
        }
      }
    }
    float tm = GD_EXCLUDED;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ki = t * 16 + 4 * g + r;
        bool ok = ki < nk;
        if (MASK2D) {
          if (ok && p.mask != nullptr) ok = p.mask[((long)b * p.Nq + (qvalid ? qi : p.Nq - 1)) * p.Nk + k0 + ki] != 0;
        } else {
          ok = ok && km[ki] != 0;
        }
        const float v = ok ? s[t][r] * p.scale_log2e : GD_EXCLUDED;
        s[t][r] = v;
        tm = fmaxf(tm, v);
      }
    tm = fmaxf(tm, __shfl_xor(tm, 16));
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    const float mn = fmaxf(m, tm);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    lsum *= alpha;
#pragma unroll
    for (int db = 0; db < D / 16; ++db)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[db][r] *= alpha;
    // ---- P = 2^(S - m), O^T += V^T . P^T
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nt) {
        V4 pf;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pf[r] = (T)__builtin_amdgcn_exp2f(s[t][r] - mn);
          lsum += (float)pf[r];
        }
#pragma unroll
        for (int db = 0; db < D / 16; ++db) {
          const V4 vf = *(const V4*)(vt + (db * 16 + l15) * VSTR + (t * 16 + 4 * g) * 2);
          o[db] = GdMfma<T>::k16(vf, pf, o[db]);
        }
      }
    }
  }
  if (!active) return;
  lsum += __shfl_xor(lsum, 16);
  lsum += __shfl_xor(lsum, 32);
  if (!qvalid) return;
  // ---- the lane holds d = 16 db + 4 g + 0 .. 3 of its query
  if (PARTIAL) {
    float* wb = p.ws + (((long)b * p.heads + h) * p.nchunks + c) * (long)p.Nq * (D + 2);
#pragma unroll
    for (int db = 0; db < D / 16; ++db) *(f32x4*)(wb + (long)qi * D + db * 16 + 4 * g) = o[db];
    if (g == 0) {
      wb[(long)p.Nq * D + qi] = m;
      wb[(long)p.Nq * (D + 1) + qi] = lsum;
    }
  } else {
    const float inv = 1.0f / lsum;
    char* op = p.out + ((long)b * p.o_bs + (long)qi * p.ldo + (long)h * D) * 2;
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
      V4 ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov[r] = (T)(o[db][r] * inv);
      *(V4*)(op + (db * 16 + 4 * g) * 2) = ov;
    }
  }
}

template <typename T, int D, bool MASK2D, bool PARTIAL>
__global__ __launch_bounds__(256) void attn_tiled_kernel(AtP p) { attn_tiled_body<T, D, MASK2D, PARTIAL>(p); }
// head_dim 32 under a key mask [B Nk] (the decoder's self-attention and text cross-attention): one 16x16x32 step per 16-key tile, two
// accumulator blocks
template <typename T>
__global__ __launch_bounds__(256) void attn_hd32_kernel(AtP p) { attn_tiled_body<T, 32, false, false>(p); }

// ---- thread = (sample, head, row, 4 channels): the chunks' partials in ascending order
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_fold_kernel(const float* ws, char* out, long ldo, long o_bs, int B, int heads, int Nq, int nchunks) {
  using V4 = typename Vec<T>::v4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * heads * Nq * (D / 4)) return;
  const int d4 = (int)(i % (D / 4));
  const long r = i / (D / 4);
  const int q = (int)(r % Nq);
  const long bh = r / Nq;
  const int h = (int)(bh % heads);
  const long b = bh / heads;
  const long cstride = (long)Nq * (D + 2);
  const float* wb = ws + bh * nchunks * cstride;
  float M = GD_EXCLUDED;
  for (int c = 0; c < nchunks; ++c) M = fmaxf(M, wb[c * cstride + (long)Nq * D + q]);
  float l = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nchunks; ++c) {
    const float* wc = wb + c * cstride;
    const float f = __builtin_amdgcn_exp2f(wc[(long)Nq * D + q] - M);
    l = __builtin_fmaf(f, wc[(long)Nq * (D + 1) + q], l);
    const f32x4 a = *(const f32x4*)(wc + (long)q * D + d4 * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(f, a[e], acc[e]);
  }
  const float inv = 1.0f / l;
  V4 ov;
#pragma unroll
  for (int e = 0; e < 4; ++e) ov[e] = (T)(acc[e] * inv);
  *(V4*)(out + (b * o_bs + (long)q * ldo + (long)h * D + d4 * 4) * 2) = ov;
}

bool gd_aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

template <typename T, int L>
int msd_launch(const MsdP& p, bool mask, bool box, hipStream_t s) {
  const dim3 grid((unsigned)((p.pairs + 63) / 64));
  if (box) {
    if (mask) OMG_LAUNCH((msdeform_box_kernel<T, L, true>), grid, dim3(256), 0, s, p);
    else OMG_LAUNCH((msdeform_box_kernel<T, L, false>), grid, dim3(256), 0, s, p);
  } else {
    if (mask) OMG_LAUNCH((msdeform_kernel<T, L, true>), grid, dim3(256), 0, s, p);
    else OMG_LAUNCH((msdeform_kernel<T, L, false>), grid, dim3(256), 0, s, p);
  }
  return omg_check_launch("msdeform_attn");
}

template <typename T>
int msd_dispatch(const MsdP& p, int L, bool mask, bool box, hipStream_t s) {
  switch (L) {
    case 1: return msd_launch<T, 1>(p, mask, box, s);
    case 2: return msd_launch<T, 2>(p, mask, box, s);
    case 3: return msd_launch<T, 3>(p, mask, box, s);
    default: return msd_launch<T, 4>(p, mask, box, s);
  }
}

template <typename T, int D, bool MASK2D, bool PARTIAL>
int at_launch(const AtP& p, int B, hipStream_t s) {
  const dim3 grid((unsigned)((p.Nq + 63) / 64), (unsigned)(p.heads * p.nchunks), (unsigned)B);
  OMG_LAUNCH((attn_tiled_kernel<T, D, MASK2D, PARTIAL>), grid, dim3(256), 0, s, p);
  return omg_check_launch("attn_tiled");
}

// the checks the two halves of the bi-attention share; 0 = nothing to do
int bi_check(const char* what, int dtype, int B, int heads, int N, int T, const void* vis, int64_t ld_vis, int64_t vis_bs, const void* txt,
             int64_t ld_txt, int64_t txt_bs, const void* out, int64_t ldo, int64_t o_bs, int rows_out) {
  (void)what;
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_attn_bi: dtype");
  OMG_REQUIRE(B >= 0 && N >= 0 && T >= 0 && heads >= 1, "omg_attn_bi: B, N, T >= 0, heads >= 1");
  OMG_REQUIRE(T <= 256, "omg_attn_bi: T at most 256");
  OMG_REQUIRE(B <= 65535 && heads <= 64 && N <= (1 << 24), "omg_attn_bi: B at most 65535, heads at most 64, N at most 2^24");
  if (B == 0 || N == 0 || T == 0) return 1;
  OMG_REQUIRE(vis && txt && out, "omg_attn_bi: null operand");
  const int64_t hd = (int64_t)heads * 256;
  OMG_REQUIRE(ld_vis >= 2 * hd && ld_txt >= 2 * hd && ldo >= hd, "omg_attn_bi: row stride below 2 heads 256 (q | v, k | v) / heads 256 (out)");
  OMG_REQUIRE(ld_vis % 8 == 0 && ld_txt % 8 == 0 && ldo % 8 == 0 && vis_bs % 8 == 0 && txt_bs % 8 == 0 && o_bs % 8 == 0,
              "omg_attn_bi: row and batch strides multiples of 8");
  OMG_REQUIRE(vis_bs >= (int64_t)(N - 1) * ld_vis + 2 * hd && txt_bs >= (int64_t)(T - 1) * ld_txt + 2 * hd &&
              o_bs >= (int64_t)(rows_out - 1) * ldo + hd, "omg_attn_bi: batch stride below a sample's rows");
  OMG_REQUIRE(gd_aligned16(vis) && gd_aligned16(txt) && gd_aligned16(out), "omg_attn_bi: 16-byte aligned operands");
  return 0;
}

// omg_msdeform_attn (box = false) and omg_msdeform_attn_box: one set of checks
int msd_entry(const omg_msdeform_args* a, void* stream, bool box) {
  OMG_REQUIRE(a != nullptr, "omg_msdeform_attn: null args");
  OMG_REQUIRE(a->dtype == OMG_F16 || a->dtype == OMG_BF16, "omg_msdeform_attn: dtype");
  OMG_REQUIRE(a->head_dim == 32, "omg_msdeform_attn: head_dim 32");
  OMG_REQUIRE(a->points == 4, "omg_msdeform_attn: points 4");
  OMG_REQUIRE(a->L >= 1 && a->L <= 4, "omg_msdeform_attn: 1 to 4 levels");
  OMG_REQUIRE(a->B >= 0 && a->N >= 0 && a->Nq >= 0 && a->heads >= 1 && a->heads <= 1024, "omg_msdeform_attn: B, N, Nq >= 0, 1 <= heads <= 1024");
  if (a->B == 0 || a->Nq == 0) return OMG_OK;
  OMG_REQUIRE(a->value && a->ow && a->ref && a->out, "omg_msdeform_attn: null operand");
  OMG_REQUIRE((int64_t)a->B * a->N <= (1LL << 31) && (int64_t)a->B * a->Nq * a->heads <= (1LL << 36), "omg_msdeform_attn: B N at most 2^31, B Nq heads at most 2^36");
  for (int l = 0; l < a->L; ++l) {
    OMG_REQUIRE(a->H[l] >= 1 && a->W[l] >= 1 && a->H[l] <= 16384 && a->W[l] <= 16384, "omg_msdeform_attn: level sizes 1 .. 16384");
    OMG_REQUIRE(a->start[l] >= 0 && (int64_t)a->start[l] + (int64_t)a->H[l] * a->W[l] <= a->N, "omg_msdeform_attn: a level's rows beyond N");
  }
  const int64_t hd = (int64_t)a->heads * 32;
  OMG_REQUIRE(a->ldv >= hd && a->ldo >= hd && a->ldow >= (int64_t)a->heads * a->L * 12,
              "omg_msdeform_attn: row stride below heads 32 (value, out) / heads L 12 (offsets | logits)");
  OMG_REQUIRE(a->ldv % 8 == 0 && a->ldo % 8 == 0 && a->ldow % 8 == 0, "omg_msdeform_attn: row strides multiples of 8");
  OMG_REQUIRE(gd_aligned16(a->value) && gd_aligned16(a->ow) && gd_aligned16(a->out) && (uintptr_t)a->ref % (box ? 16 : 4) == 0,
              "omg_msdeform_attn: 16-byte aligned operands");
  MsdP p;
  p.value = (const char*)a->value; p.ldv = (long)a->ldv;
  p.mask = (const unsigned char*)a->mask;
  p.ow = (const char*)a->ow; p.ldow = (long)a->ldow;
  p.ref = a->ref;
  p.out = (char*)a->out; p.ldo = (long)a->ldo;
  p.N = a->N; p.Nq = a->Nq; p.heads = a->heads;
  p.pairs = (long)a->B * a->Nq * a->heads;
  for (int l = 0; l < 4; ++l) {
    p.H[l] = l < a->L ? a->H[l] : 1; p.W[l] = l < a->L ? a->W[l] : 1; p.start[l] = l < a->L ? a->start[l] : 0;
  }
  hipStream_t s = (hipStream_t)stream;
  return a->dtype == OMG_F16 ? msd_dispatch<f16>(p, a->L, a->mask != nullptr, box, s) : msd_dispatch<bf16>(p, a->L, a->mask != nullptr, box, s);
}

}  // namespace

extern "C" int omg_msdeform_attn(const omg_msdeform_args* a, void* stream) { return msd_entry(a, stream, false); }
extern "C" int omg_msdeform_attn_box(const omg_msdeform_args* a, void* stream) { return msd_entry(a, stream, true); }

extern "C" int omg_attn_hd32(int dtype, int B, int heads, int Nq, int Nk, const void* Q, int64_t ldq, int64_t q_bstride,
                             const void* K, int64_t ldk, int64_t k_bstride, const void* V, int64_t ldv, int64_t v_bstride,
                             const uint8_t* key_mask, float scale, void* O, int64_t ldo, int64_t o_bstride, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_attn_hd32: dtype");
  OMG_REQUIRE(B >= 0 && Nq >= 0 && Nk >= 0 && heads >= 1, "omg_attn_hd32: B, Nq, Nk >= 0, heads >= 1");
  OMG_REQUIRE(B <= 65535 && heads <= 65535 && Nq <= (1 << 24) && Nk <= (1 << 24), "omg_attn_hd32: B, heads at most 65535, Nq, Nk at most 2^24");
  if (B == 0 || Nq == 0 || Nk == 0) return OMG_OK;
  OMG_REQUIRE(Q && K && V && O, "omg_attn_hd32: null operand");
  const int64_t hd = (int64_t)heads * 32;
  OMG_REQUIRE(ldq >= hd && ldk >= hd && ldv >= hd && ldo >= hd, "omg_attn_hd32: row stride below heads 32");
  OMG_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && q_bstride % 8 == 0 && k_bstride % 8 == 0 &&
              v_bstride % 8 == 0 && o_bstride % 8 == 0, "omg_attn_hd32: row and batch strides multiples of 8");
  OMG_REQUIRE(gd_aligned16(Q) && gd_aligned16(K) && gd_aligned16(V) && gd_aligned16(O), "omg_attn_hd32: 16-byte aligned operands");
  AtP p;
  p.q = (const char*)Q; p.ldq = (long)ldq; p.q_bs = (long)q_bstride;
  p.k = (const char*)K; p.ldk = (long)ldk; p.k_bs = (long)k_bstride;
  p.v = (const char*)V; p.ldv = (long)ldv; p.v_bs = (long)v_bstride;
  p.mask = key_mask;
  p.out = (char*)O; p.ldo = (long)ldo; p.o_bs = (long)o_bstride;
  p.ws = nullptr;
  p.heads = heads; p.Nq = Nq; p.Nk = Nk; p.chunk = Nk; p.nchunks = 1;
  p.scale_log2e = scale * GD_LOG2E;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((Nq + 63) / 64), (unsigned)heads, (unsigned)B);
  if (dtype == OMG_F16) OMG_LAUNCH((attn_hd32_kernel<f16>), grid, dim3(256), 0, s, p);
  else OMG_LAUNCH((attn_hd32_kernel<bf16>), grid, dim3(256), 0, s, p);
  return omg_check_launch("attn_hd32");
}

extern "C" int omg_attn_bi_vision(int dtype, int B, int heads, int N, int T, const void* vis, int64_t ld_vis, int64_t vis_bstride,
                                  const void* txt, int64_t ld_txt, int64_t txt_bstride, const uint8_t* text_mask, float scale,
                                  void* out, int64_t ldo, int64_t o_bstride, void* stream) {
  const int rc = bi_check("vision", dtype, B, heads, N, T, vis, ld_vis, vis_bstride, txt, ld_txt, txt_bstride, out, ldo, o_bstride, N);
  if (rc != 0) return rc < 0 ? rc : OMG_OK;
  const long hd = (long)heads * 256;
  AtP p;
  p.q = (const char*)vis; p.ldq = (long)ld_vis; p.q_bs = (long)vis_bstride;
  p.k = (const char*)txt; p.ldk = (long)ld_txt; p.k_bs = (long)txt_bstride;
  p.v = (const char*)txt + hd * 2; p.ldv = (long)ld_txt; p.v_bs = (long)txt_bstride;
  p.mask = text_mask;
  p.out = (char*)out; p.ldo = (long)ldo; p.o_bs = (long)o_bstride;
  p.ws = nullptr;
  p.heads = heads; p.Nq = N; p.Nk = T; p.chunk = T; p.nchunks = 1;
  p.scale_log2e = scale * GD_LOG2E;
  hipStream_t s = (hipStream_t)stream;
  return dtype == OMG_F16 ? at_launch<f16, 256, false, false>(p, B, s) : at_launch<bf16, 256, false, false>(p, B, s);
}

extern "C" int omg_attn_bi_text_chunk(int N) {
  if (N <= 0) return 64;
  const int per = (N + 63) / 64;               // at most 64 chunks ...
  return per <= 64 ? 64 : (per + 63) / 64 * 64;     // ... of whole 64-key tiles
}

extern "C" int64_t omg_attn_bi_text_ws_floats(int B, int heads, int T, int N) {
  if (B <= 0 || heads <= 0 || T <= 0 || N <= 0) return 0;
  const int chunk = omg_attn_bi_text_chunk(N);
  return (int64_t)B * heads * ((N + chunk - 1) / chunk) * T * (256 + 2);
}

extern "C" int omg_attn_bi_text(int dtype, int B, int heads, int N, int T, const void* vis, int64_t ld_vis, int64_t vis_bstride,
                                const void* txt, int64_t ld_txt, int64_t txt_bstride, const uint8_t* vision_mask, float scale,
                                float* workspace, void* out, int64_t ldo, int64_t o_bstride, void* stream) {
  const int rc = bi_check("text", dtype, B, heads, N, T, vis, ld_vis, vis_bstride, txt, ld_txt, txt_bstride, out, ldo, o_bstride, T);
  if (rc != 0) return rc < 0 ? rc : OMG_OK;
  OMG_REQUIRE(workspace != nullptr && gd_aligned16(workspace), "omg_attn_bi_text: workspace null or not 16-byte aligned");
  const long hd = (long)heads * 256;
  AtP p;
  p.q = (const char*)txt; p.ldq = (long)ld_txt; p.q_bs = (long)txt_bstride;
  p.k = (const char*)vis; p.ldk = (long)ld_vis; p.k_bs = (long)vis_bstride;
  p.v = (const char*)vis + hd * 2; p.ldv = (long)ld_vis; p.v_bs = (long)vis_bstride;
  p.mask = vision_mask;
  p.out = nullptr; p.ldo = 0; p.o_bs = 0;
  p.ws = workspace;
  p.heads = heads; p.Nq = T; p.Nk = N;
  p.chunk = omg_attn_bi_text_chunk(N);
  p.nchunks = (N + p.chunk - 1) / p.chunk;
  p.scale_log2e = scale * GD_LOG2E;
  OMG_REQUIRE((long)heads * p.nchunks <= 65535, "omg_attn_bi_text: grid limits");
  hipStream_t s = (hipStream_t)stream;
  const int rc2 = dtype == OMG_F16 ? at_launch<f16, 256, false, true>(p, B, s) : at_launch<bf16, 256, false, true>(p, B, s);
  if (rc2 != OMG_OK) return rc2;
  const long total = (long)B * heads * T * 64;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (dtype == OMG_F16) OMG_LAUNCH((attn_fold_kernel<f16, 256>), grid, dim3(256), 0, s, workspace, (char*)out, (long)ldo, (long)o_bstride, B, heads, T, p.nchunks);
  else OMG_LAUNCH((attn_fold_kernel<bf16, 256>), grid, dim3(256), 0, s, workspace, (char*)out, (long)ldo, (long)o_bstride, B, heads, T, p.nchunks);
  return omg_check_launch("attn_fold");
}

extern "C" int omg_attn_masked(int dtype, int B, int heads, int Nq, int Nk, const void* Q, int64_t ldq, int64_t q_bstride,
                               const void* K, int64_t ldk, int64_t k_bstride, const void* V, int64_t ldv, int64_t v_bstride,
                               const uint8_t* mask, float scale, void* O, int64_t ldo, int64_t o_bstride, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_attn_masked: dtype");
  OMG_REQUIRE(B >= 0 && Nq >= 0 && Nk >= 0 && heads >= 1, "omg_attn_masked: B, Nq, Nk >= 0, heads >= 1");
  OMG_REQUIRE(Nq <= 256 && Nk <= 256, "omg_attn_masked: Nq, Nk at most 256");
  OMG_REQUIRE(B <= 65535 && heads <= 65535, "omg_attn_masked: grid limits");
  if (B == 0 || Nq == 0 || Nk == 0) return OMG_OK;
  OMG_REQUIRE(Q && K && V && O, "omg_attn_masked: null operand");
  const int64_t hd = (int64_t)heads * 64;
  OMG_REQUIRE(ldq >= hd && ldk >= hd && ldv >= hd && ldo >= hd, "omg_attn_masked: row stride below heads 64");
  OMG_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && q_bstride % 8 == 0 && k_bstride % 8 == 0 &&
              v_bstride % 8 == 0 && o_bstride % 8 == 0, "omg_attn_masked: row and batch strides multiples of 8");
  OMG_REQUIRE(gd_aligned16(Q) && gd_aligned16(K) && gd_aligned16(V) && gd_aligned16(O), "omg_attn_masked: 16-byte aligned operands");
  AtP p;
  p.q = (const char*)Q; p.ldq = (long)ldq; p.q_bs = (long)q_bstride;
  p.k = (const char*)K; p.ldk = (long)ldk; p.k_bs = (long)k_bstride;
  p.v = (const char*)V; p.ldv = (long)ldv; p.v_bs = (long)v_bstride;
  p.mask = mask;
  p.out = (char*)O; p.ldo = (long)ldo; p.o_bs = (long)o_bstride;
  p.ws = nullptr;
  p.heads = heads; p.Nq = Nq; p.Nk = Nk; p.chunk = Nk; p.nchunks = 1;
  p.scale_log2e = scale * GD_LOG2E;
  hipStream_t s = (hipStream_t)stream;
  return dtype == OMG_F16 ? at_launch<f16, 64, true, false>(p, B, s) : at_launch<bf16, 64, true, false>(p, B, s);
}
