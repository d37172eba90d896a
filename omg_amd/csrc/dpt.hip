// dpt.hip — what the DPT-hybrid depth estimator (omg_amd/dpt.py) needs beside omg_gemm, omg_layernorm, omg_attn_fwd, omg_gelu_erf
// and the dense 3x3 convolution (omg_conv3x3_nhwc_ex in effvit.hip), for gfx950.  NHWC fp16 / bf16 activations, fp32 accumulation and
// statistics, one rounding at the store; every kernel is deterministic and computes a sample without regard to its neighbours in the
// batch.
//
//   omg_dpt_stem_conv              BiT's stem: 7x7, stride 2, Cin = 3, TF-"SAME" padding, NCHW pixels in (fp32 or 16-bit), NHWC out.
//   omg_groupnorm_res_act          Y = relu?(GN(X) gamma + beta [+ R]): the statistics of omg_groupnorm (gn_stats.h), the bottleneck's
//                                  residual add and ReLU in the apply pass.
//   omg_maxpool3x3s2_nhwc          3x3 stride-2 max-pool under the SAME rule with pad value 0.
//   omg_upsample2x_bilinear_nhwc   bilinear x2, align_corners = True.
//   omg_rowdot_f32                 Y[m] = relu?(X[m, :] . w + b) in fp32: the 32 -> 1 head projection.
//   omg_depth_tail                 get_depth's tail: bicubic resize of the fp32 depth, min-max normalisation, 8-bit, three channels.
#include "gn_stats.h"

namespace {

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// TF "SAME": output size ceil(n / stride), total padding max((out - 1) stride + k - n, 0), its smaller half in front
inline int same_front(int n, int k, int stride) {
  const int out = (n + stride - 1) / stride;
  const int pad = (out - 1) * stride + k - n;
  return pad > 0 ? pad / 2 : 0;
}

// ------------------------------------------------------------------------------------------------ stem convolution
// K = 7 * 7 * 3 = 147: too short for an MFMA pipeline to pay, so packed dot products (v_dot2_f32_f16 / v_dot2_f32_bf16: two
// 16-bit products into an fp32 accumulator per instruction).  k = (ky * 7 + kx) * 3 + c, padded to 148 = 74 pairs.  A block is 64
// output pixels x 4 waves; wave w computes the output channels [w Cout / 4, (w + 1) Cout / 4) of the block's pixels, so the weight
// reads from LDS are wave-uniform (broadcast) and a lane keeps its pixel's 74 input pairs in registers for all of its channels.
// Pixel values are rounded to the storage dtype as they are loaded (what a 16-bit module input would hold).
constexpr int STEM_KP = 74;

template <typename T> struct Dot2;
template <> struct Dot2<f16> {
  typedef _Float16 v2 __attribute__((ext_vector_type(2)));
  static OMG_DEV float dot(unsigned a, unsigned b, float c) { return __builtin_amdgcn_fdot2(__builtin_bit_cast(v2, a), __builtin_bit_cast(v2, b), c, false); }
};
template <> struct Dot2<bf16> {
  typedef __bf16 v2 __attribute__((ext_vector_type(2)));
  static OMG_DEV float dot(unsigned a, unsigned b, float c) { return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2, a), __builtin_bit_cast(v2, b), c, false); }
};

template <typename T> OMG_DEV unsigned short bits16(T v) { return __builtin_bit_cast(unsigned short, v); }

template <typename T, typename TIN>
__global__ __launch_bounds__(256) void stem_conv_kernel(const TIN* X, const unsigned* Wp, char* Y, int B, int H, int W, int Hout, int Wout,
                                                        int Cout, int pad_t, int pad_l) {
  extern __shared__ __attribute__((aligned(16))) unsigned stem_w[];      // [Cout][STEM_KP]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < Cout * STEM_KP; i += 256) stem_w[i] = Wp[i];
  const long M = (long)B * Hout * Wout;
  const long m = (long)blockIdx.x * 64 + lane;
  const bool live = m < M;
  const long mm = live ? m : 0;
  const int ox = (int)(mm % Wout), oy = (int)((mm / Wout) % Hout);
  const long b = mm / ((long)Wout * Hout);
  unsigned xp[STEM_KP];
  {
    unsigned short prev = 0;
#pragma unroll
    for (int k = 0; k < 2 * STEM_KP; ++k) {
      unsigned short cur = 0;
      if (k < 147) {
        const int tap = k / 3, c = k - 3 * tap;
        const int ky = tap / 7, kx = tap - 7 * ky;
        const int iy = oy * 2 - pad_t + ky, ix = ox * 2 - pad_l + kx;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) cur = bits16<T>((T)(float)X[((b * 3 + c) * H + iy) * (long)W + ix]);
      }
      if (k & 1) xp[k >> 1] = (unsigned)prev | ((unsigned)cur << 16);
      prev = cur;
    }
  }
  __syncthreads();
  if (!live) return;
  const int cpw = Cout >> 2;                                             // channels per wave, a multiple of 8
  for (int c0 = wave * cpw; c0 < (wave + 1) * cpw; c0 += 8) {
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    const unsigned* wr = stem_w + c0 * STEM_KP;
#pragma unroll
    for (int k = 0; k < STEM_KP; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = Dot2<T>::dot(xp[k], wr[e * STEM_KP + k], acc[e]);
    store8<T>(Y + (m * Cout + c0) * (long)sizeof(T), acc);
  }
}

// ------------------------------------------------------------------------------------------------ GroupNorm + residual + ReLU
// gn_apply_kernel of norm.hip with the bottleneck's tail in it: y = (x - mean) rstd gamma + beta, + r, max(., 0).
template <typename T>
__global__ __launch_bounds__(256) void gn_res_act_kernel(GnP p, const char* R, int relu) {
  __shared__ float mean_s[64], rstd_s[64];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x, b = p.b0 + blockIdx.y;
  const int C = p.C1;
  if (tid < p.G) {
    const float* mr = p.ws + (long)p.B * GN_MAX_CHUNKS * p.G * 2 + ((long)b * p.G + tid) * 2;
    mean_s[tid] = mr[0];
    rstd_s[tid] = mr[1];
  }
  __syncthreads();
  const int prow = tid / p.tpp, tv = tid - prow * p.tpp;
  if (prow >= p.pr) return;
  const int pix0 = chunk * p.ppc;
  const int pix1 = min(p.HW, pix0 + p.ppc);
  for (int v = 0; v < p.vpt; ++v) {
    const int vec = tv + v * p.tpp;
    if (vec >= p.nvec) break;
    float sc[8], mu[8], sh[8];
    {
      float ga[8];
      load8<T>(p.gamma + (long)vec * 8 * sizeof(T), ga);
      load8<T>(p.beta + (long)vec * 8 * sizeof(T), sh);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int g = (vec * 8 + e) / p.cpg;
        sc[e] = rstd_s[g] * ga[e]; mu[e] = mean_s[g];
      }
    }
    for (int pix = pix0 + prow; pix < pix1; pix += p.pr) {
      const long off = (((long)b * p.HW + pix) * C + vec * 8) * (long)sizeof(T);
      float f[8];
      load8<T>(p.X1 + off, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = (f[e] - mu[e]) * sc[e] + sh[e];
      if (R != nullptr) {
        float r[8];
        load8<T>(R + off, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] += r[e];
      }
      if (relu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = f[e] < 0.f ? 0.f : f[e];
      }
      store8<T>(p.Y + off, f);
    }
  }
}

// ------------------------------------------------------------------------------------------------ max-pool, upsample: a lane = 8 channels of one output pixel
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const char* X, char* Y, int B, int H, int W, int C, int Hout, int Wout, int pad_t, int pad_l) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int nv = C >> 3;
  if (idx >= (long)B * Hout * Wout * nv) return;
  const int v = (int)(idx % nv);
  const long pix = idx / nv;
  const int ox = (int)(pix % Wout), oy = (int)((pix / Wout) % Hout);
  const long b = pix / ((long)Wout * Hout);
  float m[8];
  bool first = true;
#pragma unroll
  for (int ty = 0; ty < 3; ++ty)
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
      const int iy = oy * 2 - pad_t + ty, ix = ox * 2 - pad_l + tx;
      float x[8];
      if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) load8<T>(X + (((b * H + iy) * W + ix) * C + v * 8) * (long)sizeof(T), x);
      else {                                                  // the pad value takes part in the maximum
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = first ? x[e] : fmaxf(m[e], x[e]);
      first = false;
    }
  store8<T>(Y + (pix * C + v * 8) * (long)sizeof(T), m);
}

// torch's upsample_bilinear2d, align_corners = True: source coordinate dst * (in - 1) / (out - 1) (0 when out == 1), the two taps
// weighted (1 - l) and l, rows first and then the two rows
template <typename T>
__global__ __launch_bounds__(256) void upsample2x_kernel(const char* X, char* Y, int B, int H, int W, int C, float sy, float sx) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int nv = C >> 3;
  const int Hout = 2 * H, Wout = 2 * W;
  if (idx >= (long)B * Hout * Wout * nv) return;
  const int v = (int)(idx % nv);
  const long pix = idx / nv;
  const int ox = (int)(pix % Wout), oy = (int)((pix / Wout) % Hout);
  const long b = pix / ((long)Wout * Hout);
  const float ry = sy * (float)oy, rx = sx * (float)ox;
  const int y0 = min((int)ry, H - 1), x0 = min((int)rx, W - 1);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float ly = ry - (float)y0, lx = rx - (float)x0;
  float a[8], c[8], d[8], e2[8], out[8];
  load8<T>(X + (((b * H + y0) * W + x0) * C + v * 8) * (long)sizeof(T), a);
  load8<T>(X + (((b * H + y0) * W + x1) * C + v * 8) * (long)sizeof(T), c);
  load8<T>(X + (((b * H + y1) * W + x0) * C + v * 8) * (long)sizeof(T), d);
  load8<T>(X + (((b * H + y1) * W + x1) * C + v * 8) * (long)sizeof(T), e2);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float top = (1.0f - lx) * a[e] + lx * c[e];
    const float bot = (1.0f - lx) * d[e] + lx * e2[e];
    out[e] = (1.0f - ly) * top + ly * bot;
  }
  store8<T>(Y + (pix * C + v * 8) * (long)sizeof(T), out);
}

// ------------------------------------------------------------------------------------------------ row dot product
// a lane = one row: C / 8 vector loads, fp32 sum in channel order (the same order for every row and batch size)
template <typename T>
__global__ __launch_bounds__(256) void rowdot_kernel(const char* X, long ldx, long M, int C, const char* w, const char* bias, int relu, float* Y) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float acc = bias != nullptr ? (float)*(const T*)bias : 0.f;
  for (int c = 0; c < C; c += 8) {
    float x[8], ww[8];
    load8<T>(X + (m * ldx + c) * (long)sizeof(T), x);
    load8<T>(w + (long)c * sizeof(T), ww);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(x[e], ww[e], acc);
  }
  Y[m] = relu && acc < 0.f ? 0.f : acc;
}

// ------------------------------------------------------------------------------------------------ get_depth's tail
// torch's upsample_bicubic2d, align_corners = False (the formula of effvit.hip's upsample_add_kernel, on one fp32 channel).  Both
// launches call this one function with contraction pinned by explicit fma, so the value whose minimum and maximum launch 1 took is
// bit for bit the value launch 2 normalises.
OMG_DEV void tail_cubic_w(float t, float (&w)[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.0f, x3 = 2.0f - t, x2 = 1.0f - t;
  w[0] = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(A, x0, -5.0f * A), x0, 8.0f * A), x0, -4.0f * A);
  w[1] = __builtin_fmaf(__builtin_fmaf(A + 2.0f, t, -(A + 3.0f)) * t, t, 1.0f);
  w[2] = __builtin_fmaf(__builtin_fmaf(A + 2.0f, x2, -(A + 3.0f)) * x2, x2, 1.0f);
  w[3] = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(A, x3, -5.0f * A), x3, 8.0f * A), x3, -4.0f * A);
}

OMG_DEV float tail_resized(const float* D, int h, int w, int oy, int ox, float sy, float sx) {
  const float ry = __builtin_fmaf(sy, (float)oy + 0.5f, -0.5f), rx = __builtin_fmaf(sx, (float)ox + 0.5f, -0.5f);
  const float fy = __builtin_floorf(ry), fx = __builtin_floorf(rx);
  float wy[4], wx[4];
  tail_cubic_w(ry - fy, wy);
  tail_cubic_w(rx - fx, wx);
  const int by = (int)fy - 1, bx = (int)fx - 1;
  float out = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int iy = min(max(by + i, 0), h - 1);
    float row = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ix = min(max(bx + j, 0), w - 1);
      row = __builtin_fmaf(D[(long)iy * w + ix], wx[j], row);
    }
    out = __builtin_fmaf(row, wy[i], out);
  }
  return out;
}

constexpr int TAIL_PPB = 2048;                        // output pixels per block of launch 1 (8 per lane)

// launch 1: (min, max) of the resized map over the block's pixels -> ws[(b * nblk + blk) * 2]
__global__ __launch_bounds__(256) void tail_minmax_kernel(const float* D, int h, int w, int H, int W, float sy, float sx, int nblk, float* ws) {
  __shared__ float smin[4], smax[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* Db = D + (long)b * h * w;
  const long HW = (long)H * W;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int i = 0; i < TAIL_PPB / 256; ++i) {
    const long px = (long)blockIdx.x * TAIL_PPB + i * 256 + tid;
    if (px < HW) {
      const float v = tail_resized(Db, h, w, (int)(px / W), (int)(px % W), sy, sx);
      mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
  if ((tid & 63) == 0) { smin[tid >> 6] = mn; smax[tid >> 6] = mx; }
  __syncthreads();
  if (tid == 0) {
    float* out = ws + ((long)b * nblk + blockIdx.x) * 2;
    out[0] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    out[1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  }
}

// launch 2: every block folds the sample's nblk partials (minimum and maximum are exact in any order), recomputes its pixels and
// writes trunc(clip((v - min) / (max - min) * 255, 0, 255)) three times.  A constant map: zeros.
__global__ __launch_bounds__(256) void tail_write_kernel(const float* D, int h, int w, int H, int W, float sy, float sx, int nblk, const float* ws,
                                                         unsigned char* out) {
  __shared__ float smin[4], smax[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int i = tid; i < nblk; i += 256) {
    const float* in = ws + ((long)b * nblk + i) * 2;
    mn = fminf(mn, in[0]); mx = fmaxf(mx, in[1]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
  if ((tid & 63) == 0) { smin[tid >> 6] = mn; smax[tid >> 6] = mx; }
  __syncthreads();
  mn = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
  mx = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  const long HW = (long)H * W;
  const long px = (long)blockIdx.x * 256 + tid;
  if (px >= HW) return;
  const float v = tail_resized(D + (long)b * h * w, h, w, (int)(px / W), (int)(px % W), sy, sx);
  // a constant map: the resize leaves rounding noise of a few 2^-24 of the value (four taps per axis, weights that sum to one only
  // up to rounding), which is not a range to stretch to 0 .. 255
  const float range = mx - mn;
  const bool flat = !(range > 0x1p-20f * fmaxf(fabsf(mn), fabsf(mx)));
  float t = flat ? 0.f : (v - mn) / range * 255.0f;
  t = fminf(fmaxf(t, 0.f), 255.0f);
  const unsigned char q = (unsigned char)(int)t;
  unsigned char* o = out + ((long)b * HW + px) * 3;
  o[0] = q; o[1] = q; o[2] = q;
}

}  // namespace

extern "C" int omg_dpt_stem_conv(int in_dtype, int dtype, const void* X, int B, int H, int W, int Cout, const void* Wp, void* Y, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_dpt_stem_conv: dtype");
  OMG_REQUIRE(in_dtype == OMG_F32 || in_dtype == dtype, "omg_dpt_stem_conv: pixel values in fp32 or in the storage dtype");
  OMG_REQUIRE(X && Wp && Y, "omg_dpt_stem_conv: null operand");
  OMG_REQUIRE(B >= 0 && H > 0 && W > 0, "omg_dpt_stem_conv: shape");
  OMG_REQUIRE(Cout > 0 && Cout % 32 == 0 && Cout <= 128, "omg_dpt_stem_conv: Cout a multiple of 32, at most 128");
  OMG_REQUIRE((uintptr_t)Wp % 4 == 0 && aligned16(Y), "omg_dpt_stem_conv: aligned operands");
  const int Hout = (H + 1) / 2, Wout = (W + 1) / 2;
  const long M = (long)B * Hout * Wout;
  if (M == 0) return OMG_OK;
  OMG_REQUIRE((M + 63) / 64 <= 0x7fffffffL, "omg_dpt_stem_conv: grid limits");
  const int pad_t = same_front(H, 7, 2), pad_l = same_front(W, 7, 2);
  const dim3 grid((unsigned)((M + 63) / 64));
  const size_t lds = (size_t)Cout * STEM_KP * 4;
  hipStream_t s = (hipStream_t)stream;
#define OMG_STEM(T_, TIN_) OMG_LAUNCH((stem_conv_kernel<T_, TIN_>), grid, dim3(256), lds, s, (const TIN_*)X, (const unsigned*)Wp, (char*)Y, B, H, W, Hout, Wout, Cout, pad_t, pad_l)
  if (dtype == OMG_F16) { if (in_dtype == OMG_F32) OMG_STEM(f16, float); else OMG_STEM(f16, f16); }
  else { if (in_dtype == OMG_F32) OMG_STEM(bf16, float); else OMG_STEM(bf16, bf16); }
#undef OMG_STEM
  return omg_check_launch("dpt_stem_conv");
}

extern "C" int omg_groupnorm_res_act(int dtype, const void* X, int B, int HW, int C, int groups, float eps, const void* gamma, const void* beta,
                                     const void* residual, int relu, float* workspace, void* Y, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_groupnorm_res_act: dtype");
  OMG_REQUIRE(X && gamma && beta && workspace && Y, "omg_groupnorm_res_act: null operand");
  OMG_REQUIRE(C > 0 && C % 8 == 0 && groups > 0 && groups <= 64 && C % groups == 0, "omg_groupnorm_res_act: channels/groups");
  OMG_REQUIRE(C / 8 <= 512, "omg_groupnorm_res_act: C <= 4096");
  OMG_REQUIRE(aligned16(X) && aligned16(gamma) && aligned16(beta) && aligned16(residual) && aligned16(Y), "omg_groupnorm_res_act: 16-byte aligned operands");
  OMG_REQUIRE(B >= 0 && HW >= 0 && B <= 65535, "omg_groupnorm_res_act: shape");
  if (B == 0 || HW == 0) return OMG_OK;
  GnP p{};
  gn_plan(p, C, 0, B, HW, groups);
  p.X1 = (const char*)X; p.X2 = nullptr;
  p.eps = eps; p.gamma = (const char*)gamma; p.beta = (const char*)beta; p.silu = 0;
  p.ws = workspace; p.Y = (char*)Y; p.b0 = 0;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = gn_stats_lds(p);
  const dim3 grid(p.nchunk, B);
  if (dtype == OMG_F16) {
    OMG_LAUNCH(gn_stats_kernel<f16>, grid, dim3(256), lds, s, p);
    OMG_LAUNCH(gn_finalize_kernel, dim3(p.G, B), dim3(64), 0, s, p);
    OMG_LAUNCH(gn_res_act_kernel<f16>, grid, dim3(256), 0, s, p, (const char*)residual, relu);
  } else {
    OMG_LAUNCH(gn_stats_kernel<bf16>, grid, dim3(256), lds, s, p);
    OMG_LAUNCH(gn_finalize_kernel, dim3(p.G, B), dim3(64), 0, s, p);
    OMG_LAUNCH(gn_res_act_kernel<bf16>, grid, dim3(256), 0, s, p, (const char*)residual, relu);
  }
  return omg_check_launch("groupnorm_res_act");
}

extern "C" int omg_maxpool3x3s2_nhwc(int dtype, const void* X, int B, int H, int W, int C, void* Y, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_maxpool3x3s2_nhwc: dtype");
  OMG_REQUIRE(X && Y, "omg_maxpool3x3s2_nhwc: null operand");
  OMG_REQUIRE(B >= 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "omg_maxpool3x3s2_nhwc: shape, C a multiple of 8");
  OMG_REQUIRE(aligned16(X) && aligned16(Y), "omg_maxpool3x3s2_nhwc: 16-byte aligned operands");
  const int Hout = (H + 1) / 2, Wout = (W + 1) / 2;
  const long total = (long)B * Hout * Wout * (C / 8);
  if (total == 0) return OMG_OK;
  OMG_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "omg_maxpool3x3s2_nhwc: grid limits");
  const dim3 grid((unsigned)((total + 255) / 256));
  const int pad_t = same_front(H, 3, 2), pad_l = same_front(W, 3, 2);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OMG_F16) OMG_LAUNCH(maxpool_kernel<f16>, grid, dim3(256), 0, s, (const char*)X, (char*)Y, B, H, W, C, Hout, Wout, pad_t, pad_l);
  else OMG_LAUNCH(maxpool_kernel<bf16>, grid, dim3(256), 0, s, (const char*)X, (char*)Y, B, H, W, C, Hout, Wout, pad_t, pad_l);
  return omg_check_launch("maxpool3x3s2_nhwc");
}

extern "C" int omg_upsample2x_bilinear_nhwc(int dtype, const void* X, int B, int H, int W, int C, void* Y, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_upsample2x_bilinear_nhwc: dtype");
  OMG_REQUIRE(X && Y, "omg_upsample2x_bilinear_nhwc: null operand");
  OMG_REQUIRE(B >= 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "omg_upsample2x_bilinear_nhwc: shape, C a multiple of 8");
  OMG_REQUIRE(H <= (1 << 20) && W <= (1 << 20), "omg_upsample2x_bilinear_nhwc: H, W");
  OMG_REQUIRE(aligned16(X) && aligned16(Y), "omg_upsample2x_bilinear_nhwc: 16-byte aligned operands");
  const long total = (long)B * 4 * H * W * (C / 8);
  if (total == 0) return OMG_OK;
  OMG_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "omg_upsample2x_bilinear_nhwc: grid limits");
  const dim3 grid((unsigned)((total + 255) / 256));
  const float sy = (float)(H - 1) / (float)(2 * H - 1), sx = (float)(W - 1) / (float)(2 * W - 1);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OMG_F16) OMG_LAUNCH(upsample2x_kernel<f16>, grid, dim3(256), 0, s, (const char*)X, (char*)Y, B, H, W, C, sy, sx);
  else OMG_LAUNCH(upsample2x_kernel<bf16>, grid, dim3(256), 0, s, (const char*)X, (char*)Y, B, H, W, C, sy, sx);
  return omg_check_launch("upsample2x_bilinear_nhwc");
}

extern "C" int omg_rowdot_f32(int dtype, const void* X, int64_t ldx, int64_t M, int C, const void* w, const void* bias, int relu, float* Y,
                              void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_rowdot_f32: dtype");
  OMG_REQUIRE(X && w && Y, "omg_rowdot_f32: null operand");
  OMG_REQUIRE(M >= 0 && C > 0 && C % 8 == 0 && ldx >= C && ldx % 8 == 0, "omg_rowdot_f32: C, ldx multiples of 8");
  OMG_REQUIRE(aligned16(X) && aligned16(w), "omg_rowdot_f32: 16-byte aligned X, w");
  if (M == 0) return OMG_OK;
  OMG_REQUIRE((M + 255) / 256 <= 0x7fffffffL, "omg_rowdot_f32: grid limits");
  const dim3 grid((unsigned)((M + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == OMG_F16) OMG_LAUNCH(rowdot_kernel<f16>, grid, dim3(256), 0, s, (const char*)X, (long)ldx, (long)M, C, (const char*)w, (const char*)bias, relu, Y);
  else OMG_LAUNCH(rowdot_kernel<bf16>, grid, dim3(256), 0, s, (const char*)X, (long)ldx, (long)M, C, (const char*)w, (const char*)bias, relu, Y);
  return omg_check_launch("rowdot_f32");
}

extern "C" int64_t omg_depth_tail_ws_floats(int B, int H, int W) {
  const long nblk = ((long)H * W + TAIL_PPB - 1) / TAIL_PPB;
  return (int64_t)B * nblk * 2;
}

extern "C" int omg_depth_tail(const float* depth, int B, int h, int w, int H, int W, float* workspace, void* out, void* stream) {
  OMG_REQUIRE(depth && workspace && out, "omg_depth_tail: null operand");
  OMG_REQUIRE(B >= 0 && B <= 65535 && h > 0 && w > 0 && H > 0 && W > 0, "omg_depth_tail: shape");
  OMG_REQUIRE(h <= 32768 && w <= 32768 && H <= 32768 && W <= 32768, "omg_depth_tail: sizes up to 32768");
  if (B == 0) return OMG_OK;
  const long HW = (long)H * W;
  const int nblk = (int)((HW + TAIL_PPB - 1) / TAIL_PPB);
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  hipStream_t s = (hipStream_t)stream;
  OMG_LAUNCH(tail_minmax_kernel, dim3(nblk, B), dim3(256), 0, s, depth, h, w, H, W, sy, sx, nblk, workspace);
  OMG_LAUNCH(tail_write_kernel, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, s, depth, h, w, H, W, sy, sx, nblk, (const float*)workspace,
             (unsigned char*)out);
  return omg_check_launch("depth_tail");
}
