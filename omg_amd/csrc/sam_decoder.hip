// sam_decoder.hip — what SAM's prompt-conditioned mask decoder (omg_amd/sam.py) needs beside omg_gemm and omg_layernorm, for gfx950:
// the segmenter's second half, between the EfficientViT image embedding (effvit.hip) and the region masks of stage 2.
//
//   omg_attn_small         softmax(Q K^T scale) V for head_dim 16 | 32: the two-way transformer's token self-attention (head_dim 32) and
//                          its two cross-attentions (head_dim 16; ~7 queries x 4096 keys, and 4096 queries x ~7 keys).  Two kernels,
//                          chosen by shape: keys split over the 256 lanes of a block with a (max, sum, acc) merge, or one query per lane
//                          with the keys in LDS.  fp32 scores, fp32 running-maximum softmax, fp32 P V, one rounding at the store.
//   omg_convt2x2_ln_gelu   the scatter half of ConvTranspose2d(k = 2, s = 2) (the GEMM half is omg_gemm): bias, optional per-pixel
//                          LayerNorm over channels (fp32 statistics), erf GELU, NHWC store at (2y + dy, 2x + dx).
//   omg_sam_mask_logits    logits[b, m, p] = sum_c hyper[b, m, c] up[b, p, c]: one pass over `up`, all M <= 4 masks per pass, fp32 out.
//   omg_sam_postprocess    postprocess_masks of the reference (bilinear to image_size^2, crop, bilinear to the original size), the
//                          intermediate recomputed per output pixel, plus the threshold.
//   omg_relu               the activation of the decoder's MLPs (omg_gemm has no ReLU epilogue).
// GELU is the erf form (gelu.h): SAM builds plain nn.GELU.
#include "common.h"

namespace {

constexpr float NEG_INF = -__builtin_inff();

// `n` (a multiple of 8) consecutive 16-bit elements -> floats
template <typename T, int D>
OMG_DEV void load_row(const char* p, float (&f)[D]) {
#pragma unroll
  for (int v = 0; v < D / 8; ++v) {
    float t[8];
    load8<T>(p + v * 16, t);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[v * 8 + e] = t[e];
  }
}

// exp(m_old - m_new) of a running maximum: a state that has seen no key yet (m_old = -inf) carries nothing
OMG_DEV float rescale(float m_old, float m_new) { return m_old == NEG_INF ? 0.0f : __expf(m_old - m_new); }

// ------------------------------------------------------------------------------------------------ attention, few queries x many keys
// One block of 256 lanes per (query, head, batch).  Lane t owns keys t, t + 256, ...: its own running (max, sum, acc[D]).  The 256
// partial triples are merged once: block maximum, every partial rescaled to it, sums over the wave by DPP / shuffles and over the four
// waves through LDS.  No key beyond Nk is ever read, so none can carry weight.
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_small_ksplit_kernel(const char* Q, long ldq, long qbs, const char* K, long ldk, long kbs,
                                                                const char* V, long ldv, long vbs, char* O, long ldo, long obs, int Nk,
                                                                float scale) {
#pragma clang fp contract(off)          // score * scale is ROUNDED before the maximum is subtracted: the largest key weighs exactly 1
  __shared__ float sM[4];
  __shared__ float sAcc[4][D + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long qi = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  float q[D];
  load_row<T, D>(Q + (b * qbs + qi * ldq + h * D) * (long)sizeof(T), q);
  const char* kp = K + (b * kbs + h * D) * (long)sizeof(T);
  const char* vp = V + (b * vbs + h * D) * (long)sizeof(T);
  float m = NEG_INF, l = 0.0f, acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.0f;
  for (int j = tid; j < Nk; j += 256) {
    float kr[D], vr[D];
    load_row<T, D>(kp + (long)j * ldk * (long)sizeof(T), kr);
    load_row<T, D>(vp + (long)j * ldv * (long)sizeof(T), vr);
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < D; ++c) s = __builtin_fmaf(q[c], kr[c], s);
    s *= scale;
    const float mn = fmaxf(m, s);
    const float corr = rescale(m, mn), p = __expf(s - mn);
    l = __builtin_fmaf(l, corr, p);
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = __builtin_fmaf(acc[c], corr, p * vr[c]);
    m = mn;
  }
  float M = m;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) M = fmaxf(M, __shfl_xor(M, off, 64));
  if (lane == 0) sM[wave] = M;
  __syncthreads();
  M = fmaxf(fmaxf(sM[0], sM[1]), fmaxf(sM[2], sM[3]));
  const float f = rescale(m, M);
  l *= f;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) l += __shfl_xor(l, off, 64);
#pragma unroll
  for (int c = 0; c < D; ++c) {
    float a = acc[c] * f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
    if (lane == 0) sAcc[wave][c] = a;
  }
  if (lane == 0) sAcc[wave][D] = l;
  __syncthreads();
  if (tid < D) {
    const float tot = (sAcc[0][tid] + sAcc[1][tid]) + (sAcc[2][tid] + sAcc[3][tid]);
    const float L = (sAcc[0][D] + sAcc[1][D]) + (sAcc[2][D] + sAcc[3][D]);
    ((T*)(O + (b * obs + qi * ldo + h * D) * (long)sizeof(T)))[tid] = (T)(tot / L);
  }
}

// ------------------------------------------------------------------------------------------------ attention, many queries x few keys
// One query per lane, one wave per block: 64 queries of one (head, batch).  Keys and values go through LDS as fp32 in tiles of 64
// (every lane reads the same row: a broadcast, no bank conflict; rows padded by 4 floats for the conflict-free fill).  Scores are taken
// eight at a time: one maximum and one rescale per eight keys.  Rows of the tile beyond Nk are filled with zeros and their scores set
// to -inf BEFORE the maximum: exp(-inf - m) is exactly 0.
constexpr int QL_KT = 64;

template <typename T, int D>
__global__ __launch_bounds__(64) void attn_small_qlane_kernel(const char* Q, long ldq, long qbs, const char* K, long ldk, long kbs,
                                                              const char* V, long ldv, long vbs, char* O, long ldo, long obs, int Nq,
                                                              int Nk, float scale) {
#pragma clang fp contract(off)          // as above; the FMAs this kernel wants are written out
  constexpr int LD = D + 4;
  __shared__ __attribute__((aligned(16))) float sK[QL_KT * LD];
  __shared__ __attribute__((aligned(16))) float sV[QL_KT * LD];
  const int lane = threadIdx.x;
  const long h = blockIdx.y, b = blockIdx.z;
  const long qi = (long)blockIdx.x * 64 + lane;
  const bool qok = qi < Nq;
  float q[D];
  load_row<T, D>(Q + (b * qbs + (qok ? qi : (long)Nq - 1) * ldq + h * D) * (long)sizeof(T), q);
  const char* kp = K + (b * kbs + h * D) * (long)sizeof(T);
  const char* vp = V + (b * vbs + h * D) * (long)sizeof(T);
  float m = NEG_INF, l = 0.0f, acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.0f;
  for (int k0 = 0; k0 < Nk; k0 += QL_KT) {
    const int n = min(QL_KT, Nk - k0);
    if (k0 > 0) __syncthreads();
    {
      float kr[D], vr[D];
      if (lane < n) {
        load_row<T, D>(kp + (long)(k0 + lane) * ldk * (long)sizeof(T), kr);
        load_row<T, D>(vp + (long)(k0 + lane) * ldv * (long)sizeof(T), vr);
      } else {
#pragma unroll
        for (int c = 0; c < D; ++c) kr[c] = vr[c] = 0.0f;
      }
#pragma unroll
      for (int c = 0; c < D; c += 4) {
        *(f32x4*)(sK + lane * LD + c) = f32x4{kr[c], kr[c + 1], kr[c + 2], kr[c + 3]};
        *(f32x4*)(sV + lane * LD + c) = f32x4{vr[c], vr[c + 1], vr[c + 2], vr[c + 3]};
      }
    }
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += 8) {
      float s[8];
      float cm = NEG_INF;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d = 0.0f;
#pragma unroll
        for (int c = 0; c < D; c += 4) {
          const f32x4 kv = *(const f32x4*)(sK + (j0 + j) * LD + c);
          d = __builtin_fmaf(q[c], kv[0], d);
          d = __builtin_fmaf(q[c + 1], kv[1], d);
          d = __builtin_fmaf(q[c + 2], kv[2], d);
          d = __builtin_fmaf(q[c + 3], kv[3], d);
        }
        s[j] = j0 + j < n ? d * scale : NEG_INF;
        cm = fmaxf(cm, s[j]);
      }
      const float mn = fmaxf(m, cm);
      const float corr = rescale(m, mn);
      l *= corr;
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] *= corr;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __expf(s[j] - mn);
        l += p;
#pragma unroll
        for (int c = 0; c < D; c += 4) {
          const f32x4 vv = *(const f32x4*)(sV + (j0 + j) * LD + c);
          acc[c] = __builtin_fmaf(p, vv[0], acc[c]);
          acc[c + 1] = __builtin_fmaf(p, vv[1], acc[c + 1]);
          acc[c + 2] = __builtin_fmaf(p, vv[2], acc[c + 2]);
          acc[c + 3] = __builtin_fmaf(p, vv[3], acc[c + 3]);
        }
      }
      m = mn;
    }
  }
  if (!qok) return;
  const float inv = 1.0f / l;
  char* op = O + (b * obs + qi * ldo + h * D) * (long)sizeof(T);
#pragma unroll
  for (int v = 0; v < D / 8; ++v) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = acc[v * 8 + e] * inv;
    store8<T>(op + v * 16, t);
  }
}

template <typename T, int D>
int attn_small_launch(int B, int heads, int Nq, int Nk, const void* Q, long ldq, long qbs, const void* K, long ldk, long kbs, const void* V,
                      long ldv, long vbs, float scale, void* O, long ldo, long obs, hipStream_t s) {
  // few queries against many keys: a block per query, the keys over its lanes.  The choice reads Nq and Nk only, never the batch.
  if (Nq <= 64 && Nk > Nq) {
    OMG_LAUNCH((attn_small_ksplit_kernel<T, D>), dim3((unsigned)Nq, (unsigned)heads, (unsigned)B), dim3(256), 0, s, (const char*)Q, ldq,
               qbs, (const char*)K, ldk, kbs, (const char*)V, ldv, vbs, (char*)O, ldo, obs, Nk, scale);
  } else {
    OMG_LAUNCH((attn_small_qlane_kernel<T, D>), dim3((unsigned)((Nq + 63) / 64), (unsigned)heads, (unsigned)B), dim3(64), 0, s,
               (const char*)Q, ldq, qbs, (const char*)K, ldk, kbs, (const char*)V, ldv, vbs, (char*)O, ldo, obs, Nq, Nk, scale);
  }
  return omg_check_launch("attn_small");
}

// ------------------------------------------------------------------------------------------------ transposed convolution: scatter
// G [B H W][ldg]: row r holds the four Cout-wide pieces (dy, dx) = (0,0) (0,1) (1,0) (1,1) of input pixel r (the GEMM against the
// weight laid out [(dy, dx, cout)][cin]).  Output pixel (2y + dy, 2x + dx) of the NHWC map Y [B, 2H, 2W, Cout] is piece (dy, dx).
OMG_DEV const char* convt_src(const char* G, long ldg, long opix, int H, int W, int Cout, size_t esz) {
  const int W2 = 2 * W, H2 = 2 * H;
  const int ox = (int)(opix % W2), oy = (int)((opix / W2) % H2);
  const long b = opix / ((long)W2 * H2);
  const long r = (b * H + (oy >> 1)) * W + (ox >> 1);
  const int p = (oy & 1) * 2 + (ox & 1);
  return G + (r * ldg + (long)p * Cout) * (long)esz;
}

// without LayerNorm: a lane = 8 channels of one output pixel
template <typename T>
__global__ __launch_bounds__(256) void convt_scatter_kernel(const char* G, long ldg, const char* bias, char* Y, long npix, int H, int W,
                                                            int Cout, int act) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int nv = Cout >> 3;
  if (idx >= npix * nv) return;
  const int v = (int)(idx % nv);
  const long opix = idx / nv;
  float x[8];
  load8<T>(convt_src(G, ldg, opix, H, W, Cout, sizeof(T)) + v * 16, x);
  if (bias != nullptr) {
    float bv[8];
    load8<T>(bias + v * 16, bv);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] += bv[e];
  }
  if (act) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = gelu_f(x[e]);
  }
  store8<T>(Y + (opix * Cout + v * 8) * (long)sizeof(T), x);
}

// with LayerNorm over the channels of a pixel: 8 lanes per output pixel, lane `sub` the 8-channel vectors sub, sub + 8, ...  Mean, then
// the centred second moment, then the output: three passes over a row that stays in cache, statistics in fp32 on the UNROUNDED
// G + bias, one rounding at the store.
template <typename T>
__global__ __launch_bounds__(256) void convt_scatter_ln_kernel(const char* G, long ldg, const char* bias, const char* gamma,
                                                               const char* beta, float eps, char* Y, long npix, int H, int W, int Cout,
                                                               int act) {
  const long gidx = ((long)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int sub = threadIdx.x & 7;
  const bool ok = gidx < npix;
  const long opix = ok ? gidx : npix - 1;                       // the whole group stays for the shuffles
  const int nv = Cout >> 3;
  const char* g = convt_src(G, ldg, opix, H, W, Cout, sizeof(T));
  auto value = [&](int v, float (&x)[8]) {
    load8<T>(g + v * 16, x);
    if (bias != nullptr) {
      float bv[8];
      load8<T>(bias + v * 16, bv);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] += bv[e];
    }
  };
  auto group_sum = [](float s) {
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    return s;
  };
  float s1 = 0.0f;
  for (int v = sub; v < nv; v += 8) {
    float x[8];
    value(v, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) s1 += x[e];
  }
  const float mean = group_sum(s1) / (float)Cout;
  float s2 = 0.0f;
  for (int v = sub; v < nv; v += 8) {
    float x[8];
    value(v, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) s2 = __builtin_fmaf(x[e] - mean, x[e] - mean, s2);
  }
  const float rstd = 1.0f / __builtin_sqrtf(group_sum(s2) / (float)Cout + eps);
  if (!ok) return;
  for (int v = sub; v < nv; v += 8) {
    float x[8], gv[8], bv[8];
    value(v, x);
    load8<T>(gamma + v * 16, gv);
    load8<T>(beta + v * 16, bv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      x[e] = __builtin_fmaf((x[e] - mean) * rstd, gv[e], bv[e]);
      if (act) x[e] = gelu_f(x[e]);
    }
    store8<T>(Y + (opix * Cout + v * 8) * (long)sizeof(T), x);
  }
}

// ------------------------------------------------------------------------------------------------ hypernetwork x upscaled embedding
// A lane = one pixel: its C channels once from HBM, M dot products against the hypernetwork rows held in LDS (uniform reads), M
// coalesced fp32 stores.
constexpr int ML_MAXC = 64, ML_MAXM = 4;

template <typename T>
__global__ __launch_bounds__(256) void mask_logits_kernel(const char* hyper, const char* up, float* out, int M, long P, int C) {
  __shared__ float sH[ML_MAXM * ML_MAXC];
  const long b = blockIdx.y;
  for (int i = threadIdx.x; i < M * C; i += 256) sH[i] = (float)((const T*)hyper)[b * M * C + i];
  __syncthreads();
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  float acc[ML_MAXM] = {0.0f, 0.0f, 0.0f, 0.0f};
  const char* u = up + (b * P + p) * C * (long)sizeof(T);
  for (int c = 0; c < C; c += 8) {
    float x[8];
    load8<T>(u + c * (long)sizeof(T), x);
#pragma unroll
    for (int mi = 0; mi < ML_MAXM; ++mi)
      if (mi < M) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[mi] = __builtin_fmaf(sH[mi * C + c + e], x[e], acc[mi]);
      }
  }
#pragma unroll
  for (int mi = 0; mi < ML_MAXM; ++mi)
    if (mi < M) out[(b * M + mi) * P + p] = acc[mi];
}

// ------------------------------------------------------------------------------------------------ postprocess_masks
// torch's upsample_bilinear2d, align_corners = False: source coordinate max(scale (dst + 0.5) - 0.5, 0) with scale = in / out in
// fp32, neighbours clamped to the last row / column, and
//     (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11).
struct Lerp { int i0, i1; float w0, w1; };
OMG_DEV Lerp lerp_at(float scale, int dst, int in) {
  const float r = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
  const int i0 = min((int)r, in - 1);
  const float w1 = r - (float)i0;
  return Lerp{i0, i0 + (i0 < in - 1 ? 1 : 0), 1.0f - w1, w1};
}
OMG_DEV float bilerp(Lerp y, Lerp x, float v00, float v01, float v10, float v11) {
  return y.w0 * (x.w0 * v00 + x.w1 * v01) + y.w1 * (x.w0 * v10 + x.w1 * v11);
}

// a lane = one pixel of the output; the four pixels of the image_size^2 intermediate it needs are interpolated on the spot
__global__ __launch_bounds__(256) void postprocess_kernel(const float* low, int Hl, int Wl, int S, int in_h, int in_w, int out_h, int out_w,
                                                          float sy1, float sx1, float sy2, float sx2, float thr, int out_u8, void* out,
                                                          long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % out_w), oy = (int)((idx / out_w) % out_h);
  const long n = idx / ((long)out_w * out_h);
  const float* src = low + n * Hl * Wl;
  const Lerp Y = lerp_at(sy2, oy, in_h), X = lerp_at(sx2, ox, in_w);
  auto mid = [&](int my, int mx) {
    const Lerp y = lerp_at(sy1, my, Hl), x = lerp_at(sx1, mx, Wl);
    return bilerp(y, x, src[(long)y.i0 * Wl + x.i0], src[(long)y.i0 * Wl + x.i1], src[(long)y.i1 * Wl + x.i0], src[(long)y.i1 * Wl + x.i1]);
  };
  const float v = bilerp(Y, X, mid(Y.i0, X.i0), mid(Y.i0, X.i1), mid(Y.i1, X.i0), mid(Y.i1, X.i1));
  if (out_u8) ((unsigned char*)out)[idx] = v > thr ? 1 : 0;
  else ((float*)out)[idx] = v;
}

template <typename T>
__global__ __launch_bounds__(256) void relu_kernel(const char* X, char* Y, long nvec) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  float x[8];
  load8<T>(X + i * 16, x);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = x[e] < 0.0f ? 0.0f : x[e];      // a NaN stays a NaN, as torch.relu keeps it
  store8<T>(Y + i * 16, x);
}

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" int omg_attn_small(int dtype, int B, int heads, int head_dim, int Nq, int Nk, const void* Q, int64_t ldq, int64_t q_bstride,
                              const void* K, int64_t ldk, int64_t k_bstride, const void* V, int64_t ldv, int64_t v_bstride, float scale,
                              void* O, int64_t ldo, int64_t o_bstride, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_attn_small: dtype");
  OMG_REQUIRE(head_dim == 16 || head_dim == 32, "omg_attn_small: head_dim 16 or 32");
  OMG_REQUIRE(Q && K && V && O, "omg_attn_small: null operand");
  OMG_REQUIRE(B >= 1 && heads >= 1 && Nq >= 1 && Nk >= 1, "omg_attn_small: B, heads, Nq, Nk >= 1");
  OMG_REQUIRE(B <= 65535 && heads <= 65535, "omg_attn_small: grid limits");
  const int64_t w = (int64_t)heads * head_dim;
  OMG_REQUIRE(ldq >= w && ldk >= w && ldv >= w && ldo >= w, "omg_attn_small: row stride below heads * head_dim");
  OMG_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "omg_attn_small: row strides multiples of 8");
  OMG_REQUIRE(q_bstride % 8 == 0 && k_bstride % 8 == 0 && v_bstride % 8 == 0 && o_bstride % 8 == 0 && q_bstride >= 0 && k_bstride >= 0 &&
                  v_bstride >= 0 && o_bstride >= 0, "omg_attn_small: batch strides non-negative multiples of 8");
  OMG_REQUIRE(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(O), "omg_attn_small: 16-byte aligned operands");
  hipStream_t s = (hipStream_t)stream;
#define OMG_AS(T_, D_) return attn_small_launch<T_, D_>(B, heads, Nq, Nk, Q, (long)ldq, (long)q_bstride, K, (long)ldk, (long)k_bstride, V, \
                                                        (long)ldv, (long)v_bstride, scale, O, (long)ldo, (long)o_bstride, s)
  if (dtype == OMG_F16) { if (head_dim == 16) OMG_AS(f16, 16); else OMG_AS(f16, 32); }
  if (head_dim == 16) OMG_AS(bf16, 16); else OMG_AS(bf16, 32);
#undef OMG_AS
}

extern "C" int omg_convt2x2_ln_gelu(int dtype, const void* G, int64_t ldg, int B, int H, int W, int Cout, const void* bias,
                                    const void* ln_gamma, const void* ln_beta, float eps, int act, void* Y, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_convt2x2_ln_gelu: dtype");
  OMG_REQUIRE(G && Y, "omg_convt2x2_ln_gelu: null operand");
  OMG_REQUIRE(B >= 0 && H > 0 && W > 0 && H <= (1 << 14) && W <= (1 << 14), "omg_convt2x2_ln_gelu: shape");
  OMG_REQUIRE(Cout > 0 && Cout % 8 == 0, "omg_convt2x2_ln_gelu: Cout a multiple of 8");
  OMG_REQUIRE(ldg >= 4 * (int64_t)Cout && ldg % 8 == 0, "omg_convt2x2_ln_gelu: ldg >= 4 Cout, a multiple of 8");
  OMG_REQUIRE((ln_gamma == nullptr) == (ln_beta == nullptr), "omg_convt2x2_ln_gelu: LayerNorm weight and bias come together");
  OMG_REQUIRE(act == 0 || act == 1, "omg_convt2x2_ln_gelu: act 0 (none) or 1 (erf GELU)");
  OMG_REQUIRE(aligned16(G) && aligned16(Y) && aligned16(bias) && aligned16(ln_gamma) && aligned16(ln_beta), "omg_convt2x2_ln_gelu: 16-byte aligned operands");
  const long npix = (long)B * 4 * H * W;
  if (npix == 0) return OMG_OK;
  const bool ln = ln_gamma != nullptr;
  const long lanes = ln ? npix * 8 : npix * (Cout / 8);
  OMG_REQUIRE((lanes + 255) / 256 <= 0x7fffffffL, "omg_convt2x2_ln_gelu: grid limits");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((lanes + 255) / 256));
  if (ln) {
    if (dtype == OMG_F16) OMG_LAUNCH(convt_scatter_ln_kernel<f16>, grid, dim3(256), 0, s, (const char*)G, (long)ldg, (const char*)bias, (const char*)ln_gamma, (const char*)ln_beta, eps, (char*)Y, npix, H, W, Cout, act);
    else OMG_LAUNCH(convt_scatter_ln_kernel<bf16>, grid, dim3(256), 0, s, (const char*)G, (long)ldg, (const char*)bias, (const char*)ln_gamma, (const char*)ln_beta, eps, (char*)Y, npix, H, W, Cout, act);
  } else {
    if (dtype == OMG_F16) OMG_LAUNCH(convt_scatter_kernel<f16>, grid, dim3(256), 0, s, (const char*)G, (long)ldg, (const char*)bias, (char*)Y, npix, H, W, Cout, act);
    else OMG_LAUNCH(convt_scatter_kernel<bf16>, grid, dim3(256), 0, s, (const char*)G, (long)ldg, (const char*)bias, (char*)Y, npix, H, W, Cout, act);
  }
  return omg_check_launch("convt2x2_ln_gelu");
}

extern "C" int omg_sam_mask_logits(int dtype, const void* hyper, const void* up, int B, int M, int64_t P, int C, float* logits, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_sam_mask_logits: dtype");
  OMG_REQUIRE(hyper && up && logits, "omg_sam_mask_logits: null operand");
  OMG_REQUIRE(B >= 1 && B <= 65535 && M >= 1 && M <= ML_MAXM && P >= 1, "omg_sam_mask_logits: B >= 1, 1 <= M <= 4, P >= 1");
  OMG_REQUIRE(C > 0 && C % 8 == 0 && C <= ML_MAXC, "omg_sam_mask_logits: C a multiple of 8, at most 64");
  OMG_REQUIRE(aligned16(up) && (uintptr_t)hyper % 2 == 0 && (uintptr_t)logits % 4 == 0, "omg_sam_mask_logits: alignment");
  OMG_REQUIRE((P + 255) / 256 <= 0x7fffffffL, "omg_sam_mask_logits: grid limits");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((P + 255) / 256), (unsigned)B);
  if (dtype == OMG_F16) OMG_LAUNCH(mask_logits_kernel<f16>, grid, dim3(256), 0, s, (const char*)hyper, (const char*)up, logits, M, (long)P, C);
  else OMG_LAUNCH(mask_logits_kernel<bf16>, grid, dim3(256), 0, s, (const char*)hyper, (const char*)up, logits, M, (long)P, C);
  return omg_check_launch("sam_mask_logits");
}

extern "C" int omg_sam_postprocess(const float* low, int N, int Hl, int Wl, int image_size, int in_h, int in_w, int out_h, int out_w,
                                   float threshold, int out_u8, void* out, void* stream) {
  OMG_REQUIRE(low && out, "omg_sam_postprocess: null operand");
  OMG_REQUIRE(N >= 0 && Hl > 0 && Wl > 0 && image_size > 0 && out_h > 0 && out_w > 0, "omg_sam_postprocess: shape");
  OMG_REQUIRE(in_h > 0 && in_w > 0 && in_h <= image_size && in_w <= image_size, "omg_sam_postprocess: input_size within image_size");
  OMG_REQUIRE(Hl <= (1 << 14) && Wl <= (1 << 14) && image_size <= (1 << 14) && out_h <= (1 << 14) && out_w <= (1 << 14), "omg_sam_postprocess: sides at most 16384");
  OMG_REQUIRE(out_u8 == 0 || out_u8 == 1, "omg_sam_postprocess: out_u8 0 (fp32 logits) or 1 (uint8 mask)");
  OMG_REQUIRE((uintptr_t)low % 4 == 0 && (out_u8 || (uintptr_t)out % 4 == 0), "omg_sam_postprocess: alignment");
  const long total = (long)N * out_h * out_w;
  if (total == 0) return OMG_OK;
  OMG_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "omg_sam_postprocess: grid limits");
  const float sy1 = (float)Hl / (float)image_size, sx1 = (float)Wl / (float)image_size;
  const float sy2 = (float)in_h / (float)out_h, sx2 = (float)in_w / (float)out_w;
  OMG_LAUNCH(postprocess_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, low, Hl, Wl, image_size, in_h, in_w,
             out_h, out_w, sy1, sx1, sy2, sx2, threshold, out_u8, out, total);
  return omg_check_launch("sam_postprocess");
}

extern "C" int omg_relu(int dtype, const void* X, void* Y, int64_t n, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_relu: dtype");
  OMG_REQUIRE(X && Y, "omg_relu: null operand");
  OMG_REQUIRE(n >= 0 && n % 8 == 0, "omg_relu: n a multiple of 8");
  OMG_REQUIRE(aligned16(X) && aligned16(Y), "omg_relu: 16-byte aligned operands");
  if (n == 0) return OMG_OK;
  const long nvec = n / 8;
  OMG_REQUIRE((nvec + 255) / 256 <= 0x7fffffffL, "omg_relu: grid limits");
  const dim3 grid((unsigned)((nvec + 255) / 256));
  if (dtype == OMG_F16) OMG_LAUNCH(relu_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)X, (char*)Y, nvec);
  else OMG_LAUNCH(relu_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)X, (char*)Y, nvec);
  return omg_check_launch("relu");
}
