// effvit.hip — the convolutional part of the EfficientViT-SAM image encoder (omg_amd/efficientvit.py) for gfx950: what sits round
// LiteMLA (litemla.hip) in the segmenter between the two stages.  NHWC fp16 / bf16 activations, BatchNorm already folded into weight
// and bias on the host, fp32 accumulation, one rounding at the store.
//
//   omg_conv3x3_nhwc_act   dense 3x3 convolution, stride 1 | 2, padding 1, as an implicit GEMM on the 16-bit MFMA: the stem (Cin = 3),
//                          ResBlock and FusedMBConv.spatial_conv (Cin = 32, 64, 128, 256 ...).  Epilogue: bias, GELU, residual.
//   omg_dwconv3x3_act      depthwise 3x3, stride 1 | 2: MBConv.depth_conv.  GELU on the output and, optionally, on the INPUT as it is
//                          loaded (the activation of the 1x1 inverted_conv in front of it, whose GEMM has no tanh-GELU epilogue).
//   omg_upsample_add_nhwc  bicubic (a = -0.75, align_corners = False: torch.nn.functional.interpolate) resize of one neck input onto the
//                          neck grid, added to what is already there.
// GELU is the tanh form throughout: the reference builds nn.GELU(approximate="tanh") (models/nn/act.py).
#include "common.h"

namespace {

// x Phi(x) ~ x sigmoid(2 sqrt(2 / pi) (x + 0.044715 x^3)): one exp, one hardware reciprocal
OMG_DEV float gelu_tanh_f(float x) {
  const float u = x * __builtin_fmaf(0.044715f * x, x, 1.0f);
  return x * __builtin_amdgcn_rcpf(1.0f + __expf(-1.5957691216057308f * u));
}

// ------------------------------------------------------------------------------------------------ dense 3x3, implicit GEMM
// D[cout][pixel] = sum_k W[cout][k] X[pixel][k], k = (tap, cin) with cin padded to a multiple of 8 (zeros), in 16-byte vectors of 8
// channels of one tap.  A block of 4 waves owns 128 output pixels x 32 NT output channels; wave w the pixels 32 w .. 32 w + 31.  The
// weight fragment is the MFMA's A operand and the pixel fragment its B operand, so that a lane ends up with ONE pixel and runs of 4
// consecutive output channels: 8-byte NHWC stores, no exchange.  K advances 32 at a time through two LDS buffers: the global loads of
// chunk k + 1 are in flight while chunk k is multiplied; one barrier per chunk.
// LDS rows are 64 data bytes + 16 of padding: the 16-byte slot of (row r, vector v) starts at dword 20 r + 4 v, and 20 r mod 64 runs
// through all sixteen multiples of 4 for 16 consecutive rows — a ds_read_b128 of 16 lanes touches every bank once.
constexpr int C3_BM = 128;
constexpr int C3_ROWB = 80;

template <typename T, int NT, bool VEC>
__global__ __launch_bounds__(256) void conv3x3_kernel(const char* X, const char* Wt, const char* bias, const char* res, char* Y, int B,
                                                      int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int stride, int act,
                                                      int pad_t, int pad_l, int relu_in) {
  using v8 = typename Vec<T>::v8;
  constexpr int BN = 32 * NT;
  constexpr int WL = (BN * 4 + 255) / 256;                  // weight vectors per thread and chunk
  __shared__ __attribute__((aligned(16))) char sX[2][C3_BM * C3_ROWB];
  __shared__ __attribute__((aligned(16))) char sW[2][BN * C3_ROWB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const long M = (long)B * Hout * Wout;
  const long m0 = (long)blockIdx.x * C3_BM;
  const int n0 = blockIdx.y * BN;
  const int CinP = (Cin + 7) & ~7;
  const int KV = 9 * (CinP >> 3);                           // 16-byte vectors along K
  const int nchunks = (KV + 3) >> 2;

  // loader role: vector `vec` of rows tid / 4 and tid / 4 + 64 (pixels), tid / 4 (+ 64) (weights)
  const int vec = tid & 3, lrow = tid >> 2;
  long xbase[2];
  int iy0[2], ix0[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long m = m0 + lrow + 64 * i;
    if (m < M) {
      const int ox = (int)(m % Wout), oy = (int)((m / Wout) % Hout);
      const long b = m / ((long)Wout * Hout);
      xbase[i] = b * Hin * Win;
      iy0[i] = oy * stride - pad_t;
      ix0[i] = ox * stride - pad_l;
    } else {
      xbase[i] = 0;
      iy0[i] = -0x40000000;                                 // every tap lands outside the image: zeros
      ix0[i] = 0;
    }
  }
  u32x4 rx[2], rw[WL];
  auto fetch = [&](int kc) {
    const int kv = kc * 4 + vec;
    const bool kok = kv < KV;
    const int tap = kok ? (kv * 8) / CinP : 0;
    const int c0 = kv * 8 - tap * CinP;
    const int ty = tap / 3, tx = tap - 3 * ty;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int iy = iy0[i] + ty, ix = ix0[i] + tx;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (kok && (unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win) {
        const long pix = xbase[i] + (long)iy * Win + ix;
        if constexpr (VEC) {
          v = *(const u32x4*)(X + (pix * Cin + c0) * (long)sizeof(T));
        } else {                                            // Cin < 8 (the RGB stem): K zero-padded here, element by element
          v8 e;
#pragma unroll
          for (int c = 0; c < 8; ++c) e[c] = c < Cin ? ((const T*)X)[pix * Cin + c] : (T)0.0f;
          v = __builtin_bit_cast(u32x4, e);
        }
        if (relu_in) {                                      // max(x, 0) on the sign bits of the eight 16-bit values (fp16 and bf16 alike)
#pragma unroll
          for (int d = 0; d < 4; ++d) v[d] &= ~(((v[d] >> 15) & 0x00010001u) * 0xffffu);
        }
      }
      rx[i] = v;
    }
#pragma unroll
    for (int j = 0; j < WL; ++j) {
      const int r = lrow + 64 * j;
      const int n = n0 + r;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (kok && r < BN && n < Cout) {
        const long wo = ((long)n * 9 + tap) * Cin;
        if constexpr (VEC) {
          v = *(const u32x4*)(Wt + (wo + c0) * (long)sizeof(T));
        } else {
          v8 e;
#pragma unroll
          for (int c = 0; c < 8; ++c) e[c] = c < Cin ? ((const T*)Wt)[wo + c] : (T)0.0f;
          v = __builtin_bit_cast(u32x4, e);
        }
      }
      rw[j] = v;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *(u32x4*)(sX[buf] + (lrow + 64 * i) * C3_ROWB + vec * 16) = rx[i];
#pragma unroll
    for (int j = 0; j < WL; ++j)
      if (lrow + 64 * j < BN) *(u32x4*)(sW[buf] + (lrow + 64 * j) * C3_ROWB + vec * 16) = rw[j];
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int kc = 0; kc < nchunks; ++kc) {
    const int buf = kc & 1;
    const bool more = kc + 1 < nchunks;
    if (more) fetch(kc + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const v8 xf = *(const v8*)(sX[buf] + (wave * 32 + l31) * C3_ROWB + (kk * 2 + hi) * 16);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const v8 wf = *(const v8*)(sW[buf] + (j * 32 + l31) * C3_ROWB + (kk * 2 + hi) * 16);
        acc[j] = Vec<T>::mfma32(wf, xf, acc[j]);
      }
    }
    if (more) stash(buf ^ 1);
    __syncthreads();
  }

  // register r of acc[j]: output channel n0 + 32 j + 8 (r >> 2) + 4 hi + (r & 3) of pixel m0 + 32 wave + l31
  const long m = m0 + wave * 32 + l31;
  if (m >= M) return;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = n0 + j * 32 + g * 8 + hi * 4;
      if (c >= Cout) continue;                              // Cout % 8 == 0: a run of 4 is inside or outside as a whole
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[j][g * 4 + e];
      if (bias != nullptr) {
        const typename Vec<T>::v4 bv = *(const typename Vec<T>::v4*)(bias + (long)c * sizeof(T));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (float)bv[e];
      }
      if (act == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_tanh_f(v[e]);
      } else if (act == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];
      }
      if (res != nullptr) {
        const typename Vec<T>::v4 rv = *(const typename Vec<T>::v4*)(res + (m * Cout + c) * (long)sizeof(T));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
      }
      typename Vec<T>::v4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
      *(typename Vec<T>::v4*)(Y + (m * Cout + c) * (long)sizeof(T)) = o;
    }
}

template <typename T>
int conv3x3_launch(const void* X, const void* Wt, const void* bias, const void* res, void* Y, int B, int Hin, int Win, int Cin, int Hout,
                   int Wout, int Cout, int stride, int act, int pad_t, int pad_l, int relu_in, hipStream_t s) {
  const long M = (long)B * Hout * Wout;
  const unsigned gx = (unsigned)((M + C3_BM - 1) / C3_BM);
#define OMG_C3(NT_, VEC_)                                                                                                              \
  OMG_LAUNCH((conv3x3_kernel<T, NT_, VEC_>), dim3(gx, (unsigned)((Cout + 32 * NT_ - 1) / (32 * NT_))), dim3(256), 0, s, (const char*)X, \
             (const char*)Wt, (const char*)bias, (const char*)res, (char*)Y, B, Hin, Win, Cin, Hout, Wout, Cout, stride, act, pad_t, pad_l, relu_in)
  const bool vec = Cin % 8 == 0;
  if (Cout <= 32) { if (vec) OMG_C3(1, true); else OMG_C3(1, false); }
  else if (Cout <= 64) { if (vec) OMG_C3(2, true); else OMG_C3(2, false); }
  else { if (vec) OMG_C3(4, true); else OMG_C3(4, false); }
#undef OMG_C3
  return omg_check_launch("conv3x3_nhwc_act");
}

// ------------------------------------------------------------------------------------------------ depthwise 3x3
// a lane = 8 channels of one output pixel (16-byte accesses); HBM-bound streaming, fp32 accumulation
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const char* X, long ldx, const char* Wt, const char* bias, char* Y, long ldy, int B,
                                                        int Hin, int Win, int Hout, int Wout, int C, int stride, int act) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;          // over B * Hout * Wout * (C / 8)
  const int nv = C >> 3;
  if (idx >= (long)B * Hout * Wout * nv) return;
  const int v = (int)(idx % nv);
  const long pix = idx / nv;
  const int ox = (int)(pix % Wout), oy = (int)((pix / Wout) % Hout);
  const long b = pix / ((long)Wout * Hout);
  float acc[8];
  if (bias != nullptr) load8<T>(bias + (long)v * 8 * sizeof(T), acc);
  else {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  }
#pragma unroll
  for (int ty = 0; ty < 3; ++ty) {
    const int iy = oy * stride - 1 + ty;
    if ((unsigned)iy >= (unsigned)Hin) continue;
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
      const int ix = ox * stride - 1 + tx;
      if ((unsigned)ix >= (unsigned)Win) continue;
      float xv[8], wv[8];
      load8<T>(X + (((b * Hin + iy) * Win + ix) * ldx + v * 8) * (long)sizeof(T), xv);
      load8<T>(Wt + ((long)(ty * 3 + tx) * C + v * 8) * (long)sizeof(T), wv);
      if (act & 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = gelu_tanh_f(xv[e]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(xv[e], wv[e], acc[e]);
    }
  }
  if (act & 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = gelu_tanh_f(acc[e]);
  }
  store8<T>(Y + (pix * ldy + v * 8) * (long)sizeof(T), acc);
}

// ------------------------------------------------------------------------------------------------ bicubic upsample + add
// torch's upsample_bicubic2d, align_corners = False: source coordinate (dst + 0.5) in / out - 0.5, four taps per axis with the cubic
// convolution weights for a = -0.75, tap indices clamped to the image.  Rows are interpolated along x first, then along y.
OMG_DEV void cubic_w(float t, float (&w)[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.0f, x3 = 2.0f - t, x2 = 1.0f - t;
  w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
  w[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

template <typename T>
__global__ __launch_bounds__(256) void upsample_add_kernel(const char* X, char* Y, int B, int Hin, int Win, int C, int Hout, int Wout,
                                                           float sy, float sx, int accumulate) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;          // over B * Hout * Wout * (C / 8)
  const int nv = C >> 3;
  if (idx >= (long)B * Hout * Wout * nv) return;
  const int v = (int)(idx % nv);
  const long pix = idx / nv;
  const int ox = (int)(pix % Wout), oy = (int)((pix / Wout) % Hout);
  const long b = pix / ((long)Wout * Hout);
  const float ry = sy * ((float)oy + 0.5f) - 0.5f, rx = sx * ((float)ox + 0.5f) - 0.5f;
  const float fy = __builtin_floorf(ry), fx = __builtin_floorf(rx);
  float wy[4], wx[4];
  cubic_w(ry - fy, wy);
  cubic_w(rx - fx, wx);
  const int by = (int)fy - 1, bx = (int)fx - 1;
  float out[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int iy = min(max(by + i, 0), Hin - 1);
    float row[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) row[e] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ix = min(max(bx + j, 0), Win - 1);
      float xv[8];
      load8<T>(X + ((((b * Hin + iy) * Win + ix) * C) + v * 8) * (long)sizeof(T), xv);
#pragma unroll
      for (int e = 0; e < 8; ++e) row[e] = __builtin_fmaf(xv[e], wx[j], row[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = __builtin_fmaf(row[e], wy[i], out[e]);
  }
  char* yp = Y + (pix * C + v * 8) * (long)sizeof(T);
  if (accumulate) {
    float yv[8];
    load8<T>(yp, yv);
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] += yv[e];
  }
  store8<T>(yp, out);
}

}  // namespace

extern "C" int omg_conv3x3_nhwc_act(int dtype, const void* X, int B, int Hin, int Win, int Cin, int Cout, int stride, const void* Wt,
                                    const void* bias, int act, const void* residual, void* Y, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_conv3x3_nhwc_act: dtype");
  OMG_REQUIRE(X && Wt && Y, "omg_conv3x3_nhwc_act: null operand");
  OMG_REQUIRE(stride == 1 || stride == 2, "omg_conv3x3_nhwc_act: stride 1 or 2");
  OMG_REQUIRE(B >= 0 && Hin > 0 && Win > 0, "omg_conv3x3_nhwc_act: shape");
  OMG_REQUIRE(Cin > 0 && (Cin % 8 == 0 || Cin < 8), "omg_conv3x3_nhwc_act: Cin a multiple of 8, or below 8");
  OMG_REQUIRE(Cout > 0 && Cout % 8 == 0, "omg_conv3x3_nhwc_act: Cout a multiple of 8");
  OMG_REQUIRE(act == 0 || act == 1, "omg_conv3x3_nhwc_act: act 0 (none) or 1 (tanh GELU)");
  OMG_REQUIRE((long)9 * ((Cin + 7) / 8 * 8) < (1 << 24), "omg_conv3x3_nhwc_act: Cin");
  OMG_REQUIRE(Cin % 8 != 0 || ((uintptr_t)X % 16 == 0 && (uintptr_t)Wt % 16 == 0), "omg_conv3x3_nhwc_act: 16-byte aligned X, W");
  OMG_REQUIRE((uintptr_t)Y % 8 == 0 && (uintptr_t)bias % 8 == 0 && (uintptr_t)residual % 8 == 0, "omg_conv3x3_nhwc_act: 8-byte aligned Y, bias, residual");
  const int Hout = (Hin - 1) / stride + 1, Wout = (Win - 1) / stride + 1;
  const long M = (long)B * Hout * Wout;
  if (M == 0) return OMG_OK;
  OMG_REQUIRE((M + C3_BM - 1) / C3_BM <= 0x7fffffffL && (Cout + 31) / 32 <= 65535, "omg_conv3x3_nhwc_act: grid limits");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OMG_F16) return conv3x3_launch<f16>(X, Wt, bias, residual, Y, B, Hin, Win, Cin, Hout, Wout, Cout, stride, act, 1, 1, 0, s);
  return conv3x3_launch<bf16>(X, Wt, bias, residual, Y, B, Hin, Win, Cin, Hout, Wout, Cout, stride, act, 1, 1, 0, s);
}

// The same kernel with what the DPT depth estimator (omg_amd/dpt.py) needs of it: a ReLU epilogue, ReLU of the input as it is loaded
// (the pre-activation residual unit reads x and relu(x)), and the origin of TF-"SAME" padding at stride 2: total padding
// (Hout - 1) 2 + 3 - Hin with Hout = ceil(Hin / 2), its smaller half in front — 0 in front of an even size, 1 in front of an odd one.
extern "C" int omg_conv3x3_nhwc_ex(int dtype, const void* X, int B, int Hin, int Win, int Cin, int Cout, int stride, const void* Wt,
                                   const void* bias, int act, const void* residual, int flags, void* Y, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_conv3x3_nhwc_ex: dtype");
  OMG_REQUIRE(X && Wt && Y, "omg_conv3x3_nhwc_ex: null operand");
  OMG_REQUIRE(stride == 1 || stride == 2, "omg_conv3x3_nhwc_ex: stride 1 or 2");
  OMG_REQUIRE(B >= 0 && Hin > 0 && Win > 0, "omg_conv3x3_nhwc_ex: shape");
  OMG_REQUIRE(Cin > 0 && (Cin % 8 == 0 || Cin < 8), "omg_conv3x3_nhwc_ex: Cin a multiple of 8, or below 8");
  OMG_REQUIRE(Cout > 0 && Cout % 8 == 0, "omg_conv3x3_nhwc_ex: Cout a multiple of 8");
  OMG_REQUIRE(act >= 0 && act <= 2, "omg_conv3x3_nhwc_ex: act 0 (none), 1 (tanh GELU) or 2 (ReLU)");
  OMG_REQUIRE((flags & ~3) == 0, "omg_conv3x3_nhwc_ex: flags bit 0 (ReLU of the input) | bit 1 (SAME origin)");
  OMG_REQUIRE((long)9 * ((Cin + 7) / 8 * 8) < (1 << 24), "omg_conv3x3_nhwc_ex: Cin");
  OMG_REQUIRE(Cin % 8 != 0 || ((uintptr_t)X % 16 == 0 && (uintptr_t)Wt % 16 == 0), "omg_conv3x3_nhwc_ex: 16-byte aligned X, W");
  OMG_REQUIRE((uintptr_t)Y % 8 == 0 && (uintptr_t)bias % 8 == 0 && (uintptr_t)residual % 8 == 0, "omg_conv3x3_nhwc_ex: 8-byte aligned Y, bias, residual");
  const int Hout = (Hin - 1) / stride + 1, Wout = (Win - 1) / stride + 1;      // = ceil(Hin / stride): the SAME rule's size too
  const bool same = (flags & 2) != 0 && stride == 2;
  const int pad_t = same ? (Hin & 1) : 1, pad_l = same ? (Win & 1) : 1;
  const long M = (long)B * Hout * Wout;
  if (M == 0) return OMG_OK;
  OMG_REQUIRE((M + C3_BM - 1) / C3_BM <= 0x7fffffffL && (Cout + 31) / 32 <= 65535, "omg_conv3x3_nhwc_ex: grid limits");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OMG_F16) return conv3x3_launch<f16>(X, Wt, bias, residual, Y, B, Hin, Win, Cin, Hout, Wout, Cout, stride, act, pad_t, pad_l, flags & 1, s);
  return conv3x3_launch<bf16>(X, Wt, bias, residual, Y, B, Hin, Win, Cin, Hout, Wout, Cout, stride, act, pad_t, pad_l, flags & 1, s);
}

extern "C" int omg_dwconv3x3_act(int dtype, const void* X, int64_t ldx, int B, int Hin, int Win, int C, int stride, const void* Wt,
                                 const void* bias, int act, void* Y, int64_t ldy, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_dwconv3x3_act: dtype");
  OMG_REQUIRE(X && Wt && Y, "omg_dwconv3x3_act: null operand");
  OMG_REQUIRE(stride == 1 || stride == 2, "omg_dwconv3x3_act: stride 1 or 2");
  OMG_REQUIRE(B >= 0 && Hin > 0 && Win > 0, "omg_dwconv3x3_act: shape");
  OMG_REQUIRE(C > 0 && C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && ldx >= C && ldy >= C, "omg_dwconv3x3_act: C, ldx, ldy multiples of 8");
  OMG_REQUIRE(act >= 0 && act <= 3, "omg_dwconv3x3_act: act bits 1 (GELU of the output) | 2 (GELU of the input)");
  OMG_REQUIRE((uintptr_t)X % 16 == 0 && (uintptr_t)Wt % 16 == 0 && (uintptr_t)Y % 16 == 0 && (uintptr_t)bias % 16 == 0, "omg_dwconv3x3_act: 16-byte aligned operands");
  const int Hout = (Hin - 1) / stride + 1, Wout = (Win - 1) / stride + 1;
  const long total = (long)B * Hout * Wout * (C / 8);
  if (total == 0) return OMG_OK;
  OMG_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "omg_dwconv3x3_act: grid limits");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (dtype == OMG_F16) OMG_LAUNCH(dwconv3x3_kernel<f16>, grid, dim3(256), 0, s, (const char*)X, (long)ldx, (const char*)Wt, (const char*)bias, (char*)Y, (long)ldy, B, Hin, Win, Hout, Wout, C, stride, act);
  else OMG_LAUNCH(dwconv3x3_kernel<bf16>, grid, dim3(256), 0, s, (const char*)X, (long)ldx, (const char*)Wt, (const char*)bias, (char*)Y, (long)ldy, B, Hin, Win, Hout, Wout, C, stride, act);
  return omg_check_launch("dwconv3x3_act");
}

extern "C" int omg_upsample_add_nhwc(int dtype, const void* X, int B, int Hin, int Win, int C, int Hout, int Wout, int accumulate, void* Y,
                                     void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_upsample_add_nhwc: dtype");
  OMG_REQUIRE(X && Y, "omg_upsample_add_nhwc: null operand");
  OMG_REQUIRE(B >= 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "omg_upsample_add_nhwc: shape");
  OMG_REQUIRE(C > 0 && C % 8 == 0, "omg_upsample_add_nhwc: C a multiple of 8");
  OMG_REQUIRE((uintptr_t)X % 16 == 0 && (uintptr_t)Y % 16 == 0, "omg_upsample_add_nhwc: 16-byte aligned operands");
  const long total = (long)B * Hout * Wout * (C / 8);
  if (total == 0) return OMG_OK;
  OMG_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "omg_upsample_add_nhwc: grid limits");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((total + 255) / 256));
  const float sy = (float)Hin / (float)Hout, sx = (float)Win / (float)Wout;
  if (dtype == OMG_F16) OMG_LAUNCH(upsample_add_kernel<f16>, grid, dim3(256), 0, s, (const char*)X, (char*)Y, B, Hin, Win, C, Hout, Wout, sy, sx, accumulate);
  else OMG_LAUNCH(upsample_add_kernel<bf16>, grid, dim3(256), 0, s, (const char*)X, (char*)Y, B, Hin, Win, C, Hout, Wout, sy, sx, accumulate);
  return omg_check_launch("upsample_add_nhwc");
}
