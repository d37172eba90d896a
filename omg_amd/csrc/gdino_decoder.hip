// gdino_decoder.hip — what GroundingDINO's query selection, decoder and heads (omg_amd/gdino_decoder.py) need beside omg_gemm,
// omg_layernorm, omg_relu, omg_add_inplace and, in gdino.hip, omg_attn_hd32 and omg_msdeform_attn_box, for gfx950.
//
//   omg_gdino_contrastive  GroundingDinoContrastiveEmbedding: S = X Y^T over 256 channels under the text token mask, as the padded
//                          fp32 logits [B, N, max_text_len] and / or their row maximum [B, N] (the selection's score: no [B, N, T]
//                          tensor is written).
//   omg_gdino_ref_step     the reference bookkeeping between two decoder layers: the box head's last Linear, the logit of the old
//                          reference, the sigmoid, the reference per sampled level, the sine embedding of the new reference.
//
// gd_contrastive_kernel.  A workgroup is 64 rows of X (a wave owns 16) of one sample against the text rows in LDS tiles of 64
// ([64][256]); S^T = Y X^T by v_mfma_f32_16x16x32 over 8 steps per 16-token tile, so the lane holds for its row (lane & 15) the tokens
// 4 (lane >> 4) + r of every token tile: four consecutive fp32 logits, one 16-byte store.  The fp32 accumulator is stored as it is.
// The maximum runs over exactly the numbers the logits hold (-inf on a masked token), so it is bitwise their maximum whichever of the
// two outputs is asked for.
//
// gd_ref_step_kernel.  One wave per query.  Lane i owns channels 4 i .. 4 i + 3 of the 256: four products per output (exact in
// fp32: 16-bit x 16-bit) summed in channel order, then the 64 lanes by a butterfly (xor 1, 2, .. 32): a fixed pairwise order.  Every
// lane then holds delta and forms the four coordinates itself; lane i writes channels 8 i .. 8 i + 7 of the 512-wide embedding
// (coordinate block i / 16 in the library's order y, x, w, h), sinf / cosf of the device library (no fast-math forms).
#include "common.h"

namespace {

struct CtP {
  const char* x; long ldx;               // [B N][ldx]
  const char* y; long ldy;               // [B T][ldy]
  const unsigned char* mask;             // [B T], 1 = a real token
  float* logits;                         // [B N maxT] or null
  float* rowmax;                         // [B N] or null
  int N, T, maxT;
};

template <typename T>
__global__ __launch_bounds__(256) void gd_contrastive_kernel(CtP p) {
  constexpr int D = 256, KT = 64, KSTR = D * 2 + 16, CH = D / 8;
  using V8 = typename Vec<T>::v8;
  __shared__ __attribute__((aligned(16))) char yt[KT * KSTR];
  __shared__ unsigned char km[KT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, l15 = lane & 15;
  const long b = blockIdx.y;
  const int q0 = blockIdx.x * 64 + w * 16;
  const bool active = q0 < p.N;                // wave-uniform: a wave without rows only helps to stage
  const int qi = q0 + l15;
  const bool qvalid = qi < p.N;
  const float ninf = -__builtin_inff();

  V8 xf[D / 32];
  if (active) {
    const char* xp = p.x + ((b * p.N + (qvalid ? qi : p.N - 1)) * p.ldx + g * 8) * 2;
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) xf[kk] = *(const V8*)(xp + kk * 64);
  }
  float* lrow = p.logits != nullptr ? p.logits + (b * p.N + (qvalid ? qi : 0)) * (long)p.maxT : nullptr;
  const bool wr = lrow != nullptr && qvalid;
  float mx = ninf;
  const char* yb = p.y + b * p.T * p.ldy * 2;

  for (int k0 = 0; k0 < p.T; k0 += KT) {
    const int nk = min(KT, p.T - k0);
    const int nt = (nk + 15) >> 4;
    __syncthreads();
    for (int cc = tid; cc < nt * 16 * CH; cc += 256) {
      const int i = cc / CH, ch = cc - i * CH;
      u32x4 yz = {0u, 0u, 0u, 0u};
      if (i < nk) yz = *(const u32x4*)(yb + ((long)(k0 + i) * p.ldy + ch * 8) * 2);
      *(u32x4*)(yt + i * KSTR + ch * 16) = yz;
    }
    if (tid < KT) km[tid] = (tid < nk && p.mask[b * p.T + k0 + tid] != 0) ? 1 : 0;
    __syncthreads();
    if (!active) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nt) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < D / 32; ++kk) {
          const V8 yf = *(const V8*)(yt + (t * 16 + l15) * KSTR + kk * 64 + g * 16);
          s = Vec<T>::mfma16(yf, xf[kk], s);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ki = t * 16 + 4 * g + r;
          s[r] = (ki < nk && km[ki] != 0) ? s[r] : ninf;
          mx = fmaxf(mx, s[r]);
        }
        const int col = k0 + t * 16 + 4 * g;           // maxT % 4 == 0: the four columns are inside or outside together
        if (wr && col < p.maxT) *(f32x4*)(lrow + col) = s;
      }
    }
  }
  if (!active) return;
  // the columns behind the last token tile
  if (wr)
    for (int col = ((p.T + 15) >> 4) * 16 + 4 * g; col < p.maxT; col += 16) *(f32x4*)(lrow + col) = f32x4{ninf, ninf, ninf, ninf};
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  if (p.rowmax != nullptr && qvalid && g == 0) p.rowmax[b * p.N + qi] = mx;
}

struct RsP {
  const float* ref_in;                   // [rows 4] or null
  const float* logit_in;                 // [rows 4] or null (may hold +inf)
  const float* vr;                       // [B L 2]
  const char* hd; long ldh;              // [rows][ldh] or null
  const char* w3;                        // [4 256]
  const char* b3;                        // [4]
  float* ref_out;                        // [rows 4]
  float* ref_input;                      // [rows L 4] or null
  char* emb; long lde;                   // [rows][lde] or null
  int Q, L;
  long rows;
};

OMG_DEV float gd_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <typename T>
__global__ __launch_bounds__(256) void gd_ref_step_kernel(RsP p) {
  using V4 = typename Vec<T>::v4;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.rows) return;                   // wave-uniform
  const long b = row / p.Q;
  float r[4];
  if (p.hd != nullptr) {
    const V4 h4 = *(const V4*)(p.hd + (row * p.ldh + lane * 4) * 2);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const V4 w4 = *(const V4*)(p.w3 + (o * 256 + lane * 4) * 2);
      float s = (float)h4[0] * (float)w4[0];
#pragma unroll
      for (int e = 1; e < 4; ++e) s = __builtin_fmaf((float)h4[e], (float)w4[e], s);
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
      r[o] = s + (float)((const T*)p.b3)[o];
    }
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    float base;
    if (p.logit_in != nullptr) {
      base = p.logit_in[row * 4 + o];
      r[o] = gd_sigmoid(p.hd != nullptr ? r[o] + base : base);
    } else {
      const float x = p.ref_in[row * 4 + o];
      if (p.hd != nullptr) {
        // torch.special.logit(x, eps = 1e-5): the clamp to [eps, 1 - eps] in fp32, then log(x / (1 - x))
        const float xc = fminf(fmaxf(x, 1e-5f), 1.0f - 1e-5f);
        base = logf(xc / (1.0f - xc));
        r[o] = gd_sigmoid(r[o] + base);
      } else {
        r[o] = x;
      }
    }
  }
  if (lane < 4) p.ref_out[row * 4 + lane] = lane == 0 ? r[0] : lane == 1 ? r[1] : lane == 2 ? r[2] : r[3];
  const float* vr = p.vr + b * p.L * 2;
  if (p.ref_input != nullptr && lane < p.L) {
    const float vx = vr[lane * 2], vy = vr[lane * 2 + 1];
    *(f32x4*)(p.ref_input + (row * p.L + lane) * 4) = f32x4{r[0] * vx, r[1] * vy, r[2] * vx, r[3] * vy};
  }
  if (p.emb != nullptr) {
    // encode_sinusoidal_position_embedding(ref_input[:, :, 0, :], 128): blocks y, x, w, h; channel i of a block is
    // sin (i even) / cos (i odd) of coord 2 pi / 10000^(2 (i / 2) / 128)
    const int blk = lane >> 4;
    const float vx = vr[0], vy = vr[1];
    const float coord = blk == 0 ? r[1] * vy : blk == 1 ? r[0] * vx : blk == 2 ? r[2] * vx : r[3] * vy;
    const float a = coord * 6.283185307179586f;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      const int i2 = ((lane & 15) * 8 + e) >> 1;
      const float dim_t = exp2f((float)i2 * (13.287712379549449f / 64.0f));
      const float arg = a / dim_t;
      f[e] = sinf(arg);
      f[e + 1] = cosf(arg);
    }
    store8<T>(p.emb + (row * p.lde + lane * 8) * 2, f);
  }
}

bool gdd_aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" int omg_gdino_contrastive(int dtype, int B, int N, int T, int max_text_len, const void* X, int64_t ldx, const void* Y, int64_t ldy,
                                     const uint8_t* text_mask, float* logits, float* rowmax, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_gdino_contrastive: dtype");
  OMG_REQUIRE(B >= 0 && N >= 0 && T >= 1, "omg_gdino_contrastive: B, N >= 0, T >= 1");
  OMG_REQUIRE(max_text_len <= 256 && T <= max_text_len, "omg_gdino_contrastive: T <= max_text_len <= 256");
  OMG_REQUIRE(max_text_len % 4 == 0, "omg_gdino_contrastive: max_text_len a multiple of 4");
  OMG_REQUIRE(B <= 65535 && N <= (1 << 24), "omg_gdino_contrastive: B at most 65535, N at most 2^24");
  if (B == 0 || N == 0) return OMG_OK;
  OMG_REQUIRE(X && Y && text_mask, "omg_gdino_contrastive: null operand");
  OMG_REQUIRE(logits != nullptr || rowmax != nullptr, "omg_gdino_contrastive: neither logits nor rowmax");
  OMG_REQUIRE(ldx >= 256 && ldy >= 256 && ldx % 8 == 0 && ldy % 8 == 0, "omg_gdino_contrastive: row strides multiples of 8, at least 256");
  OMG_REQUIRE(gdd_aligned16(X) && gdd_aligned16(Y) && gdd_aligned16(logits) && (uintptr_t)rowmax % 4 == 0,
              "omg_gdino_contrastive: 16-byte aligned operands");
  CtP p;
  p.x = (const char*)X; p.ldx = (long)ldx;
  p.y = (const char*)Y; p.ldy = (long)ldy;
  p.mask = text_mask; p.logits = logits; p.rowmax = rowmax;
  p.N = N; p.T = T; p.maxT = max_text_len;
  const dim3 grid((unsigned)((N + 63) / 64), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OMG_F16) OMG_LAUNCH((gd_contrastive_kernel<f16>), grid, dim3(256), 0, s, p);
  else OMG_LAUNCH((gd_contrastive_kernel<bf16>), grid, dim3(256), 0, s, p);
  return omg_check_launch("gdino_contrastive");
}

extern "C" int omg_gdino_ref_step(int dtype, int B, int Q, int L, const float* ref_in, const float* logit_in, const float* valid_ratios,
                                  const void* Hd, int64_t ldh, const void* W3, const void* b3, float* ref_out, float* ref_input,
                                  void* emb, int64_t lde, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_gdino_ref_step: dtype");
  OMG_REQUIRE(B >= 0 && Q >= 0 && L >= 1 && L <= 4, "omg_gdino_ref_step: B, Q >= 0, 1 to 4 levels");
  OMG_REQUIRE((int64_t)B * Q <= (1LL << 31), "omg_gdino_ref_step: B Q at most 2^31");
  if (B == 0 || Q == 0) return OMG_OK;
  OMG_REQUIRE((ref_in != nullptr) != (logit_in != nullptr), "omg_gdino_ref_step: exactly one of ref_in and logit_in");
  OMG_REQUIRE(valid_ratios && ref_out, "omg_gdino_ref_step: null operand");
  if (Hd != nullptr) {
    OMG_REQUIRE(W3 && b3, "omg_gdino_ref_step: a hidden state without the last Linear");
    OMG_REQUIRE(ldh >= 256 && ldh % 4 == 0 && (uintptr_t)Hd % 8 == 0 && (uintptr_t)W3 % 8 == 0 && (uintptr_t)b3 % 2 == 0,
                "omg_gdino_ref_step: hidden rows of at least 256, stride a multiple of 4, 8-byte aligned");
  }
  OMG_REQUIRE(emb == nullptr || (lde >= 512 && lde % 8 == 0 && gdd_aligned16(emb)), "omg_gdino_ref_step: embedding rows of at least 512, 16-byte aligned");
  OMG_REQUIRE(gdd_aligned16(ref_input) && (uintptr_t)ref_out % 4 == 0 && (uintptr_t)valid_ratios % 4 == 0 &&
              (uintptr_t)ref_in % 4 == 0 && (uintptr_t)logit_in % 4 == 0, "omg_gdino_ref_step: aligned fp32 operands");
  RsP p;
  p.ref_in = ref_in; p.logit_in = logit_in; p.vr = valid_ratios;
  p.hd = (const char*)Hd; p.ldh = (long)ldh; p.w3 = (const char*)W3; p.b3 = (const char*)b3;
  p.ref_out = ref_out; p.ref_input = ref_input; p.emb = (char*)emb; p.lde = (long)lde;
  p.Q = Q; p.L = L; p.rows = (long)B * Q;
  const dim3 grid((unsigned)((p.rows + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OMG_F16) OMG_LAUNCH((gd_ref_step_kernel<f16>), grid, dim3(256), 0, s, p);
  else OMG_LAUNCH((gd_ref_step_kernel<bf16>), grid, dim3(256), 0, s, p);
  return omg_check_launch("gdino_ref_step");
}
