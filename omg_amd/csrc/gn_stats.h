// gn_stats.h — the statistics half of the NHWC GroupNorm, shared by norm.hip (omg_groupnorm, omg_groupnorm_mx8) and dpt.hip
// (omg_groupnorm_res_act): the launch geometry, the pivoted (mean, M2) partial sums per pixel chunk and their fixed-order fp64 fold.
// Each translation unit applies the statistics with a kernel of its own.
#pragma once
#include "common.h"

namespace {

constexpr int GN_MAX_CHUNKS = 1024;    // partial-sum chunks per sample (64 until round 2: a 1024x1024x128 VAE map then ran on 128 workgroups)

struct GnP {
  const char* X1; int C1; const char* X2; int C2;
  int B, HW, G, cpg, nvec, tpp, vpt, pr, nchunk, ppc, b0;
  float eps; const char* gamma; const char* beta; int silu;
  float* ws; char* Y;
  char* Q; unsigned char* S; long P;       // MX8 output: e4m3 bytes [B*HW][Cq] + scale bytes [(Cq/128)][P][4], P = B*HW
  int Cq;                                  // C rounded up to a multiple of 128: the pad channels are written as zeros (scale byte 0)
};

template <typename T>
OMG_DEV void gn_load(const GnP& p, int b, int pix, int vec, float (&f)[8]) {
  const int c = vec * 8;
  const char* src = (c < p.C1) ? p.X1 + (((long)b * p.HW + pix) * p.C1 + c) * (long)sizeof(T)
                               : p.X2 + (((long)b * p.HW + pix) * p.C2 + (c - p.C1)) * (long)sizeof(T);
  load8<T>(src, f);
}

// One element of [x1 | x2] as fp32 (the pivots of the statistics pass).
template <typename T>
OMG_DEV float gn_load1(const GnP& p, int b, int pix, int c) {
  const T* src = (c < p.C1) ? (const T*)p.X1 + ((long)b * p.HW + pix) * p.C1 + c
                            : (const T*)p.X2 + ((long)b * p.HW + pix) * p.C2 + (c - p.C1);
  return (float)*src;
}

// Statistics of one pixel chunk.  The sums are SHIFTED: every channel c of the chunk has a pivot P_c, the median of the channel's
// values at the chunk's first, middle and last pixel; a lane accumulates d = x - P_c and d * d in fp32, and the block turns them
// into (mean, M2 = sum (x - mean)^2) per group.  Plain sum x / sum x^2 in fp32 lost var = E[x^2] - mean^2 to cancellation once
// |mean| >> std (fp32 outputs off by 0.7 to 9 at mean / std = 1000).  The pivot is an element of the channel, so M2_c >= (P_c - mean_c)^2 and the
// cancellation left in Q - S^2 / n is bounded by n * 2^-24 of M2_c whatever the pivot happens to be; the median keeps a single
// outlier (a first pixel far from the rest) from being it, which would spend that bound.  The fold over rows and channels runs in
// fp64 in a fixed order.
// Workspace per (sample, chunk, group): {mean - P_bg, M2}, P_bg = the same median over the sample's first, middle and last pixel
// at the first channel of the group: stored relative to an element of the group, the chunk mean keeps its precision in a float;
// chunk 0 leaves P_bg in the (mean, rstd) slot for gn_finalize.
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(GnP p) {
  extern __shared__ float lds[];            // [pr][C] shifted sums, [pr][C] shifted sums of squares, [C] pivots
  const int C = p.C1 + p.C2;
  const int tid = threadIdx.x;
  const int prow = tid / p.tpp, tv = tid - prow * p.tpp;
  const int chunk = blockIdx.x, b = p.b0 + blockIdx.y;
  const int pix0 = chunk * p.ppc;
  const int pix1 = min(p.HW, pix0 + p.ppc);
  float* piv_s = lds + 2 * p.pr * C;
  if (prow < p.pr) {
    // one of the lane's (at most two) channel vectors at a time: its sums and pivots are the only accumulators alive in the pixel loop
    for (int v = 0; v < p.vpt; ++v) {
      const int vec = tv + v * p.tpp;
      if (vec >= p.nvec) break;
      float s[8], q[8], pv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
      {      // pivot: the median of the chunk's first, middle and last pixel — the same three cache lines for every pixel row
        float pm[8], pl[8];
        gn_load<T>(p, b, pix0, vec, pv);
        gn_load<T>(p, b, (pix0 + pix1) >> 1, vec, pm);
        gn_load<T>(p, b, pix1 - 1, vec, pl);
#pragma unroll
        for (int e = 0; e < 8; ++e) pv[e] = __builtin_amdgcn_fmed3f(pv[e], pm[e], pl[e]);
      }
      // four pixels per trip: four independent 16-byte loads in flight per lane (one load per trip left the kernel latency-bound
      // at 0.8-2 TB/s); the accumulation order over pixels is unchanged
      for (int pix = pix0 + prow; pix < pix1; pix += 4 * p.pr) {
        float f[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int px = pix + u * p.pr;
          if (px < pix1) gn_load<T>(p, b, px, vec, f[u]);
          else {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[u][e] = pv[e];      // past the chunk: d = 0
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int e = 0; e < 8; ++e) { const float d = f[u][e] - pv[e]; s[e] += d; q[e] += d * d; }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        lds[prow * C + vec * 8 + e] = s[e];
        lds[(p.pr + prow) * C + vec * 8 + e] = q[e];
        if (prow == 0) piv_s[vec * 8 + e] = pv[e];
      }
    }
  }
  __syncthreads();
  if (tid < p.G) {
    const double npx = (double)(pix1 - pix0), inv = 1.0 / npx;
    const double pbg = (double)__builtin_amdgcn_fmed3f(gn_load1<T>(p, b, 0, tid * p.cpg), gn_load1<T>(p, b, p.HW >> 1, tid * p.cpg), gn_load1<T>(p, b, p.HW - 1, tid * p.cpg));
    // channel c: mean_c = P_c + S / n, M2_c = Q - S^2 / n; the group: M2 = sum_c M2_c + n * sum_c (mean_c - mean)^2, the second sum
    // about the first channel's mean (r0) so that it does not cancel either
    double r0 = 0.0, a1 = 0.0, a2 = 0.0, m2 = 0.0;
    for (int c = tid * p.cpg; c < (tid + 1) * p.cpg; ++c) {
      double ss = 0.0, qq = 0.0;
      for (int r = 0; r < p.pr; ++r) { ss += (double)lds[r * C + c]; qq += (double)lds[(p.pr + r) * C + c]; }
      const double dm = ((double)piv_s[c] - pbg) + ss * inv;
      if (c == tid * p.cpg) r0 = dm;
      const double e = dm - r0;
      a1 += e; a2 += e * e;
      m2 += qq - ss * ss * inv;
    }
    m2 += npx * (a2 - a1 * a1 / (double)p.cpg);
    float* out = p.ws + (((long)b * GN_MAX_CHUNKS + chunk) * p.G + tid) * 2;
    out[0] = (float)(r0 + a1 / (double)p.cpg);
    out[1] = (float)(m2 > 0.0 ? m2 : 0.0);
    if (chunk == 0) p.ws[(long)p.B * GN_MAX_CHUNKS * p.G * 2 + ((long)b * p.G + tid) * 2] = (float)pbg;
  }
}

// One wave per (group, sample): merges the chunk partials {mean_k - P_bg, M2_k} (n_k = the chunk's pixels x channels per group) in a
// FIXED order (lane l takes chunks l, l + 64, ...; then a butterfly whose pairing does not depend on the data) in fp64:
//   mean = sum n_k mean_k / n,  M2 = sum M2_k + sum n_k (mean_k - mean)^2     (Chan et al.; the second sum about chunk 0's mean)
// and leaves (mean, rstd) behind the partials in the workspace.  Until round 2
// every block of gn_apply did this fold itself, 32 threads walking all the partials one dependent load after the other: with up to
// 1024 chunks per sample that serial prologue was 80 % of the apply pass on the UNet's largest maps (4.6 ms for 4 GB of traffic).
__global__ __launch_bounds__(64) void gn_finalize_kernel(GnP p) {
  const int g = blockIdx.x, b = p.b0 + blockIdx.y;
  const int lane = threadIdx.x;
  const double r0 = (double)p.ws[(((long)b * GN_MAX_CHUNKS) * p.G + g) * 2];
  double a1 = 0.0, a2 = 0.0, m2 = 0.0;
  for (int ch = lane; ch < p.nchunk; ch += 64) {
    const float* in = p.ws + (((long)b * GN_MAX_CHUNKS + ch) * p.G + g) * 2;
    const double nk = (double)(min(p.HW, (ch + 1) * p.ppc) - ch * p.ppc) * p.cpg;
    const double e = (double)in[0] - r0;
    a1 += nk * e; a2 += nk * e * e; m2 += (double)in[1];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    a1 += __shfl_xor(a1, o);
    a2 += __shfl_xor(a2, o);
    m2 += __shfl_xor(m2, o);
  }
  if (lane == 0) {
    const double n = (double)p.HW * p.cpg;
    float* mr = p.ws + (long)p.B * GN_MAX_CHUNKS * p.G * 2 + ((long)b * p.G + g) * 2;
    const double mean = (double)mr[0] + r0 + a1 / n;      // mr[0]: P_bg, left by chunk 0 of gn_stats
    double var = (m2 + (a2 - a1 * a1 / n)) / n;
    if (var < 0.0) var = 0.0;
    mr[0] = (float)mean;
    mr[1] = (float)(1.0 / sqrt(var + (double)p.eps));
  }
}

// Geometry of one call: lanes per pixel, pixel rows per block, pixel chunks per sample.  X1 / X2, eps, gamma, beta, ws and the outputs
// are the caller's to fill.
inline void gn_plan(GnP& p, int C1, int C2, int B, int HW, int groups) {
  const int C = C1 + C2;
  p.C1 = C1; p.C2 = C2;
  p.B = B; p.HW = HW; p.G = groups; p.cpg = C / groups; p.nvec = C / 8;
  p.vpt = p.nvec <= 256 ? 1 : 2;
  p.tpp = p.vpt == 1 ? p.nvec : (p.nvec + 1) / 2;
  p.pr = 256 / p.tpp;
  long elems = (long)HW * C;
  int nchunk = (int)((elems + 32767) / 32768);
  if (nchunk > GN_MAX_CHUNKS) nchunk = GN_MAX_CHUNKS;
  if (nchunk > HW) nchunk = HW;
  if (nchunk < 1) nchunk = 1;
  p.ppc = (HW + nchunk - 1) / nchunk;
  p.nchunk = (HW + p.ppc - 1) / p.ppc;
}
// dynamic LDS of gn_stats_kernel: <= 48 KiB (C <= 4096 has pr = 1)
inline size_t gn_stats_lds(const GnP& p) { return ((size_t)2 * p.pr + 1) * (p.C1 + p.C2) * sizeof(float); }

}  // namespace
