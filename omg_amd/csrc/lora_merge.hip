// lora_merge.hip — one weight slot of a LoRA bank, merged from the adapters' small fp32 factors (omg_lora_merge), and the row norm
// DoRA divides by (omg_lora_rownorm).  Contract: include/omg_hip.h.
//
// A wave owns a 32 x 64 tile of the slot: two 32 x 32 MFMA tiles side by side.  The plain (up . down) and the two LoHa products are
// matmul-shaped with a small reduction (the rank): they run on the f32-input MFMA, v_mfma_f32_32x32x2_f32 — exact fp32 products, per
// element one fmaf chain over the rank (cdna guide §3; gemm_f32.hip uses the same instruction), at the fp32 vector rate.  What the MFMA
// buys over packed fp32 FMAs at the same rate is operand delivery: ONE float per lane and instruction feeds 2048 multiply-adds, so the
// factors go from L2 / L1 straight into the operand registers, without an LDS stage and without the r x 8 floats per lane a
// register-blocked FMA loop would hold.
//
// Operand mapping, as in gemm_f32.hip: mfma(X, Y, acc) with X[i = lane & 31][k = lane >> 5], Y[k = lane >> 5][j = lane & 31] leaves
// D[i = 8 g + 4 hi + e][j = l31] in acc[4 g + e] of lane (l31, hi).  Here i is the COLUMN of the tile (X = down[2 t + hi][col0 + l31], a
// coalesced 128-byte read per half) and j the ROW (Y = up[n0 + l31][2 t + hi], shared by the two column tiles): a lane ends up with one
// row and runs of four consecutive columns.  The Kronecker term has no reduction: a gather and one multiply per element, indices
// advanced along the run without divisions.
// That layout is the wrong one for W and the slot (32 rows x 16 bytes per wave instruction: the first version of this kernel ran at 5x
// its memory time, whatever the term).  The sum of the terms therefore goes through a 32 x 64 fp32 tile in LDS, private to the wave, and
// comes back row-major: eight lanes cover the 64 columns of a row, a lane reads 16 bytes of W, forms W * wcoef + sum for its eight
// columns and writes 16 bytes — whole 128-byte lines of eight rows per instruction.
#include "common.h"

namespace {

constexpr int LM_CT = 2;                 // 32-column MFMA tiles per wave
constexpr int LM_WCOLS = 32 * LM_CT;     // 64 columns per wave
constexpr int LM_LDR = LM_WCOLS + 4;     // LDS row stride in floats: rows 4 banks apart, 16-byte aligned

struct LMP {
  int N, K, n_terms;
  const char* W; char* out;
  omg_lora_term t[OMG_LORA_MAX_TERMS];
};

// acc[ct][4 g + e] = sum_q up[n][q] * down[q][col0 + 32 ct + 8 g + 4 hi + e], one fmaf chain in a fixed order of q.  n is the lane's
// (clamped) row; columns beyond K and ranks beyond r contribute exact zeros.
OMG_DEV void lm_product(const float* __restrict__ up, const float* __restrict__ down, int r, int K, int n, int col0, int l31, int hi,
                        f32x16 (&acc)[LM_CT]) {
  bool col_ok[LM_CT];
  const float* dp[LM_CT];
#pragma unroll
  for (int ct = 0; ct < LM_CT; ++ct) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;
    const int col = col0 + 32 * ct + l31;
    col_ok[ct] = col < K;
    dp[ct] = down + (col_ok[ct] ? col : 0);
  }
  const float* upr = up + (long)n * r;
  // eight ranks (four MFMA steps) a trip: their operand loads are issued together, ahead of the first MFMA — one load latency a trip,
  // not one a step.  The up operand is a 32-row gather (a row a lane, r floats apart): with r % 4 == 0 a lane takes ONE 16-byte chunk of its
  // row a trip — lane half hi the ranks q0 + 4 hi .. + 3, step u contracting q0 + u and q0 + 4 + u, as gemm_f32.hip feeds its MFMAs —
  // instead of four dwords: a quarter of the L1 / L2 lines moved (the gather, not the MFMA, is what the product costs: measured 0.75 us a
  // rank on a 10240 x 1280 slot against 0.17 us of MFMA time).  Either way an element's chain has one fixed order, whatever its tile.
  const bool vec = (r & 3) == 0 && ((uintptr_t)up & 15) == 0;
  for (int q0 = 0; q0 < r; q0 += 8) {
    float y[4], x[4][LM_CT];
    if (vec) {
      const int qb = q0 + 4 * hi;
      const bool ok = qb < r;
      const int qc = ok ? qb : 0;
      const f32x4 yv = *(const f32x4*)(upr + qc);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        y[u] = ok ? yv[u] : 0.f;
#pragma unroll
        for (int ct = 0; ct < LM_CT; ++ct) {
          const float xv = dp[ct][(long)(qc + u) * K];
          x[u][ct] = (ok && col_ok[ct]) ? xv : 0.f;
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = q0 + 2 * u + hi;
        const bool ok = q < r;
        const int qc = ok ? q : 0;
        const float yv = upr[qc];
        y[u] = ok ? yv : 0.f;
#pragma unroll
        for (int ct = 0; ct < LM_CT; ++ct) {
          const float xv = dp[ct][(long)qc * K];
          x[u][ct] = (ok && col_ok[ct]) ? xv : 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int ct = 0; ct < LM_CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u][ct], y[u], acc[ct], 0, 0, 0);
  }
}

// the Kronecker delta of the lane's row n over the 16 columns it holds of the tile at col0
OMG_DEV f32x16 lm_kron(const omg_lora_term& t, int K, int n, int col0, int hi) {
  f32x16 dl;
  const int ia = n / t.c, ic = n - ia * t.c;
  const int cin = t.b * t.d;
  const float* w1 = t.f0 + (long)ia * t.b;
  const float* w2 = t.f1 + (long)ic * t.taps * t.d;
#pragma unroll
  for (int g = 0; g < 4; ++g) {           // branch-free, so that the 32 gathers of a tile are in flight together
    const int col = col0 + 8 * g + 4 * hi;
    const bool ok = col < K;              // K % 4 == 0: a run of four is inside or outside as a whole
    const int cc = ok ? col : 0;
    int tap = cc / cin;
    const int rem = cc - tap * cin;
    int ib = rem / t.d, id = rem - ib * t.d;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = w1[ib] * w2[tap * t.d + id];
      dl[4 * g + e] = ok ? v : 0.f;
      if (e < 3) {                        // the run stays below K: the indices it advances to are inside the operands
        const bool wd = ++id == t.d;
        id = wd ? 0 : id;
        ib += wd ? 1 : 0;
        const bool wb = ib == t.b;
        ib = wb ? 0 : ib;
        tap += wb ? 1 : 0;
      }
    }
  }
  return dl;
}

// d[ct][4 g + e] = delta[n][col0 + 32 ct + 8 g + 4 hi + e] of one term
OMG_DEV void lm_delta(const omg_lora_term& t, int K, int n, int col0, int l31, int hi, f32x16 (&d)[LM_CT]) {
  if (t.kind == OMG_LORA_KRON) {
#pragma unroll
    for (int ct = 0; ct < LM_CT; ++ct) d[ct] = lm_kron(t, K, n, col0 + 32 * ct, hi);
    return;
  }
  lm_product(t.f0, t.f1, t.r, K, n, col0, l31, hi, d);
  if (t.kind == OMG_LORA_HADA) {
    f32x16 d2[LM_CT];
    lm_product(t.f2, t.f3, t.r2, K, n, col0, l31, hi, d2);
#pragma unroll
    for (int ct = 0; ct < LM_CT; ++ct)
#pragma unroll
      for (int i = 0; i < 16; ++i) d[ct][i] *= d2[ct][i];
  }
}

// grid (ceil(K / 256), ceil(N / 32)), 256 threads: wave w takes the 64 columns from blockIdx.x * 256 + 64 w
template <typename T>
__global__ __launch_bounds__(256, 3) void lora_merge_kernel(LMP p) {
  __shared__ __attribute__((aligned(16))) float tile[4][32 * LM_LDR];
  __shared__ float wcoefs[4][32];
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col0 = blockIdx.x * (4 * LM_WCOLS) + w * LM_WCOLS;
  const int n0 = blockIdx.y * 32;
  float* my = tile[w];
  if (col0 < p.K) {                      // wave-uniform: a wave whose columns are all beyond K has nothing to form
    const int n = n0 + l31;
    const int nc = n < p.N ? n : p.N - 1;
    float wcoef = 1.f;
    for (int i = 0; i < p.n_terms; ++i)
      if (p.t[i].gain) wcoef += p.t[i].gain[nc] - 1.f;
    if (hi == 0) wcoefs[w][l31] = wcoef;
    f32x16 sum[LM_CT];
#pragma unroll
    for (int ct = 0; ct < LM_CT; ++ct)
#pragma unroll
      for (int i = 0; i < 16; ++i) sum[ct][i] = 0.f;
    for (int i = 0; i < p.n_terms; ++i) {
      const omg_lora_term& t = p.t[i];
      const float gs = t.gain ? t.gain[nc] * t.s : t.s;
      f32x16 d[LM_CT];
      lm_delta(t, p.K, nc, col0, l31, hi, d);
#pragma unroll
      for (int ct = 0; ct < LM_CT; ++ct)
#pragma unroll
        for (int j = 0; j < 16; ++j) sum[ct][j] = fmaf(gs, d[ct][j], sum[ct][j]);
    }
#pragma unroll
    for (int ct = 0; ct < LM_CT; ++ct)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(f32x4*)(my + l31 * LM_LDR + 32 * ct + 8 * g + 4 * hi) = f32x4{sum[ct][4 * g], sum[ct][4 * g + 1], sum[ct][4 * g + 2], sum[ct][4 * g + 3]};
  }
  __syncthreads();                       // every wave of the block arrives: nothing above returns
  if (col0 >= p.K) return;
  // row-major: eight lanes a row, eight rows an instruction, four passes
  const int rsub = lane >> 3, cc = (lane & 7) * 8;
  const int col = col0 + cc;
  if (col >= p.K) return;                // K % 8 == 0: a run of eight is inside or outside as a whole
  float wv[4][8];
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {        // the four 16-byte reads of W first: a row beyond N reads row N - 1 and stores nothing
    const int n = n0 + ps * 8 + rsub;
    load8<T>(p.W + ((long)(n < p.N ? n : p.N - 1) * p.K + col) * 2, wv[ps]);
  }
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int row = ps * 8 + rsub, n = n0 + row;
    const f32x4 s0 = *(const f32x4*)(my + row * LM_LDR + cc), s1 = *(const f32x4*)(my + row * LM_LDR + cc + 4);
    const float wc = wcoefs[w][row];
#pragma unroll
    for (int e = 0; e < 4; ++e) { wv[ps][e] = fmaf(wv[ps][e], wc, s0[e]); wv[ps][4 + e] = fmaf(wv[ps][4 + e], wc, s1[e]); }
    if (n < p.N) store8<T>(p.out + ((long)n * p.K + col) * 2, wv[ps]);
  }
}

// the lane's runs of W in the MFMA layout as floats; zeros outside the matrix (the norm kernel only reads W)
template <typename T>
OMG_DEV f32x16 lm_load_w(const char* W, int N, int K, int n, int col0, int hi) {
  f32x16 w;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int col = col0 + 8 * g + 4 * hi;
    if (n < N && col < K) {
      const typename Vec<T>::v4 v = *(const typename Vec<T>::v4*)(W + ((long)n * K + col) * 2);
#pragma unroll
      for (int e = 0; e < 4; ++e) w[4 * g + e] = (float)v[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) w[4 * g + e] = 0.f;
    }
  }
  return w;
}

// grid ceil(N / 32), 256 threads: the workgroup owns 32 whole rows; wave w takes the 64-column tiles w, w + 4, ...
template <typename T>
__global__ __launch_bounds__(256) void lora_rownorm_kernel(int N, int K, const char* W, omg_lora_term t, float* norm) {
  __shared__ float part[4][32];
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = blockIdx.x * 32 + l31;
  const int nc = n < N ? n : N - 1;
  float ss = 0.f;
  for (int col0 = w * LM_WCOLS; col0 < K; col0 += 4 * LM_WCOLS) {
    f32x16 d[LM_CT];
    lm_delta(t, K, nc, col0, l31, hi, d);
#pragma unroll
    for (int ct = 0; ct < LM_CT; ++ct) {
      const f32x16 wv = lm_load_w<T>(W, N, K, nc, col0 + 32 * ct, hi);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float v = fmaf(t.s, d[ct][j], wv[j]);
        ss = fmaf(v, v, ss);
      }
    }
  }
  ss += __shfl_xor(ss, 32);                      // the two halves of the row's columns: a + b in both lanes
  if (hi == 0) part[w][l31] = ss;
  __syncthreads();
  if (threadIdx.x < 32 && n < N) norm[n] = sqrtf(((part[0][l31] + part[1][l31]) + part[2][l31]) + part[3][l31]);
}

int lm_check_term(const omg_lora_term& t, int N, int K) {
  switch (t.kind) {
    case OMG_LORA_PLAIN:
      OMG_REQUIRE(t.r >= 1 && t.f0 && t.f1, "omg_lora: a plain term needs r >= 1, f0 [N][r] and f1 [r][K]");
      return OMG_OK;
    case OMG_LORA_HADA:
      OMG_REQUIRE(t.r >= 1 && t.r2 >= 1 && t.f0 && t.f1 && t.f2 && t.f3, "omg_lora: a hada term needs r, r2 >= 1 and four factors");
      return OMG_OK;
    case OMG_LORA_KRON:
      OMG_REQUIRE(t.a >= 1 && t.b >= 1 && t.c >= 1 && t.d >= 1 && t.taps >= 1 && t.f0 && t.f1, "omg_lora: a kron term needs positive dims, f0 [a][b] and f1 [c][taps][d]");
      OMG_REQUIRE((long)t.a * t.c == N && (long)t.taps * t.b * t.d == K, "omg_lora: kron dims must give a * c == N and taps * b * d == K");
      return OMG_OK;
    default:
      omg_set_error("omg_lora: unknown term kind");
      return OMG_EINVAL;
  }
}

}  // namespace

extern "C" int omg_lora_merge(const omg_lora_merge_args* a, void* stream) {
  OMG_REQUIRE(a != nullptr, "omg_lora_merge: null args");
  OMG_REQUIRE(a->W && a->out, "omg_lora_merge: null operand");
  OMG_REQUIRE(a->N >= 1 && a->K >= 8 && a->K % 8 == 0, "omg_lora_merge: N >= 1, K a multiple of 8");
  OMG_REQUIRE(a->n_terms >= 0 && a->n_terms <= OMG_LORA_MAX_TERMS, "omg_lora_merge: at most OMG_LORA_MAX_TERMS terms");
  OMG_REQUIRE(((uintptr_t)a->W & 15) == 0 && ((uintptr_t)a->out & 15) == 0, "omg_lora_merge: W and out must be 16-byte aligned");
  OMG_REQUIRE((a->N + 31) / 32 <= 65535, "omg_lora_merge: N beyond 32 * 65535");
  LMP p{};
  p.N = a->N; p.K = a->K; p.n_terms = a->n_terms; p.W = (const char*)a->W; p.out = (char*)a->out;
  for (int i = 0; i < a->n_terms; ++i) {
    const int rc = lm_check_term(a->terms[i], a->N, a->K);
    if (rc != OMG_OK) return rc;
    p.t[i] = a->terms[i];
  }
  const dim3 grid((a->K + 4 * LM_WCOLS - 1) / (4 * LM_WCOLS), (a->N + 31) / 32);
  if (a->dtype == OMG_F16) OMG_LAUNCH((lora_merge_kernel<f16>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else if (a->dtype == OMG_BF16) OMG_LAUNCH((lora_merge_kernel<bf16>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else { omg_set_error("omg_lora_merge: dtype must be OMG_F16 or OMG_BF16"); return OMG_EDTYPE; }
  return omg_check_launch("lora_merge");
}

extern "C" int omg_lora_rownorm(int dtype, int N, int K, const void* W, const omg_lora_term* term, float* norm, void* stream) {
  OMG_REQUIRE(W && term && norm, "omg_lora_rownorm: null operand");
  OMG_REQUIRE(N >= 1 && K >= 8 && K % 8 == 0, "omg_lora_rownorm: N >= 1, K a multiple of 8");
  OMG_REQUIRE(((uintptr_t)W & 15) == 0, "omg_lora_rownorm: W must be 16-byte aligned");
  const int rc = lm_check_term(*term, N, K);
  if (rc != OMG_OK) return rc;
  const dim3 grid((N + 31) / 32);
  if (dtype == OMG_F16) OMG_LAUNCH((lora_rownorm_kernel<f16>), grid, dim3(256), 0, (hipStream_t)stream, N, K, (const char*)W, *term, norm);
  else if (dtype == OMG_BF16) OMG_LAUNCH((lora_rownorm_kernel<bf16>), grid, dim3(256), 0, (hipStream_t)stream, N, K, (const char*)W, *term, norm);
  else { omg_set_error("omg_lora_rownorm: dtype must be OMG_F16 or OMG_BF16"); return OMG_EDTYPE; }
  return omg_check_launch("lora_rownorm");
}
