// swin.hip — what the Swin backbone (omg_amd/swin.py: transformers' SwinBackbone, GroundingDINO's image backbone) needs beside omg_gemm,
// omg_layernorm, omg_gelu_erf and omg_add_inplace, for gfx950.
//
//   omg_attn_swin         (shifted-)window attention, head_dim 32, straight from the fused QKV projection in image order: the cyclic
//                         shift, the padding to a multiple of the window, the partition into windows and its reverse are index
//                         arithmetic; the relative-position bias is looked up in the checkpoint's table and the shift mask is computed
//                         from the key's and the query's region.  Nothing but the output leaves the chip.
//   omg_swin_patch_embed  NCHW pixel values -> the rows of 4 x 4 stride-4 patches (k = (c * 4 + ky) * 4 + kx, the order of
//                         projection.weight.reshape(C, 48)), implicit zero padding at the bottom and right.
//   omg_swin_merge_ln     patch merging's 2 x 2 gather and its LayerNorm over 4 C in one pass.
//
// attn_swin_kernel.  A workgroup is ONE (window, head, sample): N = S S tokens (144 | 49), padded to NP = 144 | 64 rows of MFMA tiles.
// Token i of the window is (iy, ix) = (i / S, i % S) at position (wy S + iy, wx S + ix) of the ROLLED padded grid, which is position
// ((. + shift) mod Hp, (. + shift) mod Wp) of the padded grid; there it is a token of the image, or (beyond H x W) the pad row.
//   staging   K rows [NP][32] and V TRANSPOSED [32][NP] into LDS (tile-padding rows i >= N as zeros), the head's column of the bias table
//             as fp32 (exp2 domain) and each token's shift region;
//   scores    per wave one 16-query tile at a time: S^T = K Q^T, NT = NP / 16 products v_mfma_f32_16x16x32 (K = head_dim in one
//             instruction), the lane holding for its query (lane & 15) the keys 4 (lane >> 4) + r of every key tile: the whole row
//             of the softmax in 4 NT registers — a single pass, no running maximum;
//   softmax   fp32, exp2 domain: scale q.k + bias (+ -100 where the regions differ), tile-padding keys excluded, the maximum and the
//             sum over the lane's registers and the four lane groups, the sum on the unrounded probabilities;
//   P V       O^T = V^T P^T by v_mfma_f32_16x16x16: its B operand (4 keys per lane) IS the score layout, so P goes from the
//             accumulators to the next MFMA without leaving the registers; one rounding at the store.
// Every reduction has a fixed order inside the (window, head), so a result depends neither on the batch nor on other windows.
#include "common.h"

namespace {

constexpr float SW_LOG2E = 1.4426950408889634f;
constexpr float SW_EXCLUDED = -1e30f;

template <typename T> struct SwMfma;
template <> struct SwMfma<f16> {
  static OMG_DEV f32x4 k16(f16x4 a, f16x4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
};
template <> struct SwMfma<bf16> {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  static OMG_DEV f32x4 k16(bf16x4 a, bf16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
  }
};

struct SwinP {
  const char* qkv; long ld;              // [B H W][ld] elements: q | k | v, each heads * 32 wide
  char* out; long ldo;                   // [B H W][ldo]
  const char* table;                     // [(2 S - 1)^2][heads]
  const char* pad_kv;                    // [2 heads 32]: k | v of a position beyond the grid, or null (zeros)
  int heads, H, W, Hp, Wp, shift, nwx;
  float scale_log2e;
};

// region of a coordinate of the rolled padded axis of length n: [0, n - S) | [n - S, n - shift) | [n - shift, n)
OMG_DEV int sw_band(int c, int n, int S, int shift) { return (c >= n - S ? 1 : 0) + (c >= n - shift ? 1 : 0); }

template <typename T, int S>
__global__ __launch_bounds__(S == 12 ? 192 : 256) void attn_swin_kernel(SwinP p) {
  constexpr int D = 32;
  constexpr int N = S * S;
  constexpr int NT = (N + 15) / 16;            // 9 | 4 tiles of 16 tokens
  constexpr int NP = NT * 16;
  constexpr int NW = S == 12 ? 3 : 4;          // waves: 3 query tiles each | one each
  constexpr int NTHR = NW * 64;
  constexpr int KSTR = D * 2 + 16;             // K row, bytes: sixteen consecutive rows start on different 16-byte slots
  constexpr int VSTR = NP * 2 + 16;            // V^T row, bytes
  constexpr int TS = 2 * S - 1;
  using V8 = typename Vec<T>::v8;
  using V4 = typename Vec<T>::v4;
  __shared__ __attribute__((aligned(16))) char kt[NP * KSTR];
  __shared__ __attribute__((aligned(16))) char vt[D * VSTR];
  __shared__ float tab[TS * TS];
  __shared__ int tok[NP];                      // row of the token in the sample, -1: beyond the grid (the pad row), -2: tile padding
  __shared__ int reg[NP];                      // shift region 0 .. 8
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, l15 = lane & 15;
  const int h = blockIdx.y, b = blockIdx.z;
  const int wy = blockIdx.x / p.nwx, wx = blockIdx.x - wy * p.nwx;
  const long hd = (long)p.heads * D;
  const char* base = p.qkv + (long)b * p.H * p.W * p.ld * 2;

  // ---- the window's tokens
  for (int i = tid; i < NP; i += NTHR) {
    int t = -2, r = 0;
    if (i < N) {
      const int iy = i / S, ix = i - iy * S;
      const int ry = wy * S + iy, rx = wx * S + ix;
      int y = ry + p.shift, x = rx + p.shift;
      if (y >= p.Hp) y -= p.Hp;
      if (x >= p.Wp) x -= p.Wp;
      t = (y < p.H && x < p.W) ? y * p.W + x : -1;
      if (p.shift > 0) r = 3 * sw_band(ry, p.Hp, S, p.shift) + sw_band(rx, p.Wp, S, p.shift);
    }
    tok[i] = t;
    reg[i] = r;
  }
  // ---- the head's column of the bias table, fp32, exp2 domain
  for (int i = tid; i < TS * TS; i += NTHR) tab[i] = (float)((const T*)p.table)[(long)i * p.heads + h] * SW_LOG2E;
  __syncthreads();

  // ---- K rows and V^T: chunk c = (token i, 8 channels ch) of k and of v
  for (int c = tid; c < NP * 4; c += NTHR) {
    const int i = c >> 2, ch = c & 3;
    const int t = tok[i];
    u32x4 kz = {0u, 0u, 0u, 0u}, vz = {0u, 0u, 0u, 0u};
    if (t >= 0) {
      const char* src = base + ((long)t * p.ld + hd + (long)h * D + ch * 8) * 2;
      kz = *(const u32x4*)src;
      vz = *(const u32x4*)(src + hd * 2);
    } else if (t == -1 && p.pad_kv != nullptr) {
      const char* src = p.pad_kv + ((long)h * D + ch * 8) * 2;
      kz = *(const u32x4*)src;
      vz = *(const u32x4*)(src + hd * 2);
    }
    *(u32x4*)(kt + i * KSTR + ch * 16) = kz;
    const V8 v8 = __builtin_bit_cast(V8, vz);
#pragma unroll
    for (int e = 0; e < 8; ++e) *(T*)(vt + (ch * 8 + e) * VSTR + i * 2) = v8[e];
  }
  __syncthreads();

  for (int qt = w; qt < NT; qt += NW) {
    // ---- the lane's query: a query beyond the grid or the window is computed as a copy of the sample's first token and never stored
    const int qi = qt * 16 + l15;
    const int qtok = tok[qi];
    const int qreg = reg[qi];
    const bool valid = qtok >= 0;
    const int qiy = qi < N ? qi / S : 0, qix = qi < N ? qi - qiy * S : 0;      // tile padding: any entry of the table
    const V8 qf = *(const V8*)(base + ((long)(valid ? qtok : 0) * p.ld + (long)h * D + g * 8) * 2);

    // ---- S^T = K . Q^T per key tile; register r of tile t is key 16 t + 4 g + r
    f32x4 s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const V8 kf = *(const V8*)(kt + (t * 16 + l15) * KSTR + g * 16);
      s[t] = Vec<T>::mfma16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f});
    }
    // ---- exp2 domain: scale q.k + bias (+ mask); keys of the tile padding excluded
    float m = SW_EXCLUDED;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ki = t * 16 + 4 * g + r;
        float v = SW_EXCLUDED;
        if (ki < N) {
          const int kiy = ki / S, kix = ki - kiy * S;
          v = __builtin_fmaf(s[t][r], p.scale_log2e, tab[(qiy - kiy + S - 1) * TS + (qix - kix + S - 1)]);
          if (p.shift > 0 && reg[ki] != qreg) v += -100.0f * SW_LOG2E;
        }
        s[t][r] = v;
        m = fmaxf(m, v);
      }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    // ---- P = 2^(S - m), O^T += V^T . P^T
    float l = 0.f;
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      V4 pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[t][r] - m);
        l += e;
        pf[r] = (T)e;
      }
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const V4 vf = *(const V4*)(vt + (db * 16 + l15) * VSTR + (t * 16 + 4 * g) * 2);
        o[db] = SwMfma<T>::k16(vf, pf, o[db]);
      }
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (!valid) continue;
    const float inv = 1.0f / l;
    // ---- the lane holds d = 16 db + 4 g + 0 .. 3 of its query
    char* op = p.out + (((long)b * p.H * p.W + qtok) * p.ldo + (long)h * D) * 2;
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      V4 ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov[r] = (T)(o[db][r] * inv);
      *(V4*)(op + (db * 16 + 4 * g) * 2) = ov;
    }
  }
}

// ---- patch rows: thread = (patch, chunk j of 8 columns); column k = 8 j + e is (c, ky, kx) = (k / 16, (k / 4) & 3, k & 3); k >= 48: zero
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void swin_patch_kernel(const TI* X, char* Y, int B, int H, int W, int Hg, int Wg, int nch, long ldy) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)B * Hg * Wg * nch;
  if (i >= total) return;
  const int j = (int)(i % nch);
  const long row = i / nch;
  const int gx = (int)(row % Wg);
  const long r2 = row / Wg;
  const int gy = (int)(r2 % Hg), b = (int)(r2 / Hg);
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = 8 * j + e;
    const int c = k >> 4, y = gy * 4 + ((k >> 2) & 3), x = gx * 4 + (k & 3);
    f[e] = (k < 48 && y < H && x < W) ? (float)X[(((long)b * 3 + c) * H + y) * W + x] : 0.f;
  }
  store8<TO>(Y + (row * ldy + 8 * j) * 2, f);
}

// ---- merge + LayerNorm: a wave per output row, NCH chunks of 8 channels per lane held in registers; chunk q of the row is channels
// 8 q .. of quarter q / (C / 8): quarters (dy, dx) = (0,0), (1,0), (0,1), (1,1)
template <typename T, int NCH>
__global__ __launch_bounds__(256) void swin_merge_ln_kernel(const char* X, char* Y, const char* gamma, const char* beta, int B, int H, int W, int C,
                                                            int H2, int W2, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * H2 * W2) return;
  const int ox = (int)(row % W2);
  const long r2 = row / W2;
  const int oy = (int)(r2 % H2), b = (int)(r2 / H2);
  const int cq = C / 8, nq = 4 * cq;
  float x[NCH][8];
  float sum = 0.f;
#pragma unroll
  for (int n = 0; n < NCH; ++n) {
    const int q = n * 64 + lane;
#pragma unroll
    for (int e = 0; e < 8; ++e) x[n][e] = 0.f;
    if (q < nq) {
      const int quarter = q / cq, cc = q - quarter * cq;
      const int y = 2 * oy + (quarter & 1), xx = 2 * ox + (quarter >> 1);
      if (y < H && xx < W) load8<T>(X + ((((long)b * H + y) * W + xx) * C + cc * 8) * 2, x[n]);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += x[n][e];
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  const float mean = sum / (float)(4 * C);
  float sq = 0.f;
#pragma unroll
  for (int n = 0; n < NCH; ++n)
    if (n * 64 + lane < nq) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = x[n][e] - mean; sq += d * d; }
    }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sq += __shfl_xor(sq, o);
  const float rstd = 1.0f / sqrtf(sq / (float)(4 * C) + eps);
#pragma unroll
  for (int n = 0; n < NCH; ++n) {
    const int q = n * 64 + lane;
    if (q < nq) {
      float ga[8], be[8], y[8];
      load8<T>(gamma + (long)q * 16, ga);
      load8<T>(beta + (long)q * 16, be);
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = (x[n][e] - mean) * rstd * ga[e] + be[e];
      store8<T>(Y + (row * 4 * C + (long)q * 8) * 2, y);
    }
  }
}

bool sw_aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

template <typename T, int S>
int swin_launch(const SwinP& p, dim3 grid, hipStream_t s) {
  OMG_LAUNCH((attn_swin_kernel<T, S>), grid, dim3(S == 12 ? 192 : 256), 0, s, p);
  return omg_check_launch("attn_swin");
}

template <typename TI, typename TO>
int patch_launch(const void* X, void* Y, int B, int H, int W, int Hg, int Wg, int nch, long ldy, hipStream_t s) {
  const long total = (long)B * Hg * Wg * nch;
  OMG_LAUNCH((swin_patch_kernel<TI, TO>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const TI*)X, (char*)Y, B, H, W, Hg, Wg, nch, ldy);
  return omg_check_launch("swin_patch_embed");
}

template <typename T, int NCH>
int merge_launch(const void* X, void* Y, const void* ga, const void* be, int B, int H, int W, int C, int H2, int W2, float eps, hipStream_t s) {
  const long rows = (long)B * H2 * W2;
  OMG_LAUNCH((swin_merge_ln_kernel<T, NCH>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, (const char*)X, (char*)Y, (const char*)ga,
             (const char*)be, B, H, W, C, H2, W2, eps);
  return omg_check_launch("swin_merge_ln");
}

}  // namespace

extern "C" int omg_attn_swin(int dtype, int B, int H, int W, int heads, int window, int shift, const void* qkv, int64_t ld,
                             const void* table, const void* pad_kv, float scale, void* out, int64_t ldo, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_attn_swin: dtype");
  OMG_REQUIRE(window == 7 || window == 12, "omg_attn_swin: window 7 or 12");
  OMG_REQUIRE(shift == 0 || shift == window / 2, "omg_attn_swin: shift 0 or window / 2");
  OMG_REQUIRE(B >= 0 && H >= 0 && W >= 0 && heads >= 1, "omg_attn_swin: B, H, W >= 0, heads >= 1");
  if (B == 0 || H == 0 || W == 0) return OMG_OK;
  OMG_REQUIRE(qkv && table && out, "omg_attn_swin: null operand");
  OMG_REQUIRE(H <= 16384 && W <= 16384 && (long)H * W <= (1L << 24), "omg_attn_swin: H, W at most 16384 and H * W at most 2^24");
  OMG_REQUIRE(B <= 65535 && heads <= 65535, "omg_attn_swin: grid limits");
  const int64_t hd = (int64_t)heads * 32;
  OMG_REQUIRE(ld >= 3 * hd && ldo >= hd, "omg_attn_swin: row stride below 3 heads 32 (qkv) / heads 32 (out)");
  OMG_REQUIRE(ld % 8 == 0 && ldo % 8 == 0, "omg_attn_swin: row strides multiples of 8");
  OMG_REQUIRE(sw_aligned16(qkv) && sw_aligned16(pad_kv) && sw_aligned16(out) && (uintptr_t)table % 2 == 0, "omg_attn_swin: 16-byte aligned operands");
  SwinP p;
  p.qkv = (const char*)qkv; p.ld = (long)ld;
  p.out = (char*)out; p.ldo = (long)ldo;
  p.table = (const char*)table; p.pad_kv = (const char*)pad_kv;
  p.heads = heads; p.H = H; p.W = W; p.shift = shift;
  const int nwy = (H + window - 1) / window;
  p.nwx = (W + window - 1) / window;
  p.Hp = nwy * window; p.Wp = p.nwx * window;
  p.scale_log2e = scale * SW_LOG2E;
  const dim3 grid((unsigned)(nwy * p.nwx), (unsigned)heads, (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OMG_F16) return window == 12 ? swin_launch<f16, 12>(p, grid, s) : swin_launch<f16, 7>(p, grid, s);
  return window == 12 ? swin_launch<bf16, 12>(p, grid, s) : swin_launch<bf16, 7>(p, grid, s);
}

extern "C" int omg_swin_patch_embed(int in_dtype, int dtype, const void* X, int B, int H, int W, void* Y, int64_t ldy, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_swin_patch_embed: dtype");
  OMG_REQUIRE(in_dtype == OMG_F32 || in_dtype == dtype, "omg_swin_patch_embed: pixel values in fp32 or the storage dtype");
  OMG_REQUIRE(B >= 0 && H >= 0 && W >= 0, "omg_swin_patch_embed: B, H, W >= 0");
  if (B == 0 || H == 0 || W == 0) return OMG_OK;
  OMG_REQUIRE(X && Y, "omg_swin_patch_embed: null operand");
  OMG_REQUIRE(ldy >= 48 && ldy % 8 == 0 && ldy <= 4096, "omg_swin_patch_embed: row stride a multiple of 8, at least 48");
  OMG_REQUIRE(sw_aligned16(Y), "omg_swin_patch_embed: 16-byte aligned output");
  const int Hg = (H + 3) / 4, Wg = (W + 3) / 4, nch = (int)(ldy / 8);
  OMG_REQUIRE(((long)B * Hg * Wg * nch + 255) / 256 <= 0x7fffffffL, "omg_swin_patch_embed: grid limits");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OMG_F16) return in_dtype == OMG_F32 ? patch_launch<float, f16>(X, Y, B, H, W, Hg, Wg, nch, (long)ldy, s)
                                                   : patch_launch<f16, f16>(X, Y, B, H, W, Hg, Wg, nch, (long)ldy, s);
  return in_dtype == OMG_F32 ? patch_launch<float, bf16>(X, Y, B, H, W, Hg, Wg, nch, (long)ldy, s)
                             : patch_launch<bf16, bf16>(X, Y, B, H, W, Hg, Wg, nch, (long)ldy, s);
}

extern "C" int omg_swin_merge_ln(int dtype, const void* X, int B, int H, int W, int C, const void* gamma, const void* beta, float eps,
                                 void* Y, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_swin_merge_ln: dtype");
  OMG_REQUIRE(B >= 0 && H >= 0 && W >= 0, "omg_swin_merge_ln: B, H, W >= 0");
  OMG_REQUIRE(C >= 8 && C % 8 == 0 && C <= 1024, "omg_swin_merge_ln: C a multiple of 8, at most 1024");
  if (B == 0 || H == 0 || W == 0) return OMG_OK;
  OMG_REQUIRE(X && Y && gamma && beta, "omg_swin_merge_ln: null operand");
  OMG_REQUIRE(sw_aligned16(X) && sw_aligned16(Y) && sw_aligned16(gamma) && sw_aligned16(beta), "omg_swin_merge_ln: 16-byte aligned operands");
  const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
  OMG_REQUIRE(((long)B * H2 * W2 + 3) / 4 <= 0x7fffffffL, "omg_swin_merge_ln: grid limits");
  hipStream_t s = (hipStream_t)stream;
  const int nch = (4 * C / 8 + 63) / 64;     // chunks per lane: 1 .. 8
#define OMG_SM(T_) \
  do { \
    if (nch <= 1) return merge_launch<T_, 1>(X, Y, gamma, beta, B, H, W, C, H2, W2, eps, s); \
    if (nch <= 2) return merge_launch<T_, 2>(X, Y, gamma, beta, B, H, W, C, H2, W2, eps, s); \
    if (nch <= 4) return merge_launch<T_, 4>(X, Y, gamma, beta, B, H, W, C, H2, W2, eps, s); \
    return merge_launch<T_, 8>(X, Y, gamma, beta, B, H, W, C, H2, W2, eps, s); \
  } while (0)
  if (dtype == OMG_F16) OMG_SM(f16);
  OMG_SM(bf16);
#undef OMG_SM
}
