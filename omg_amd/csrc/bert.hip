// bert.hip — what the BERT text encoder of GroundingDINO (omg_amd/bert.py) needs beside omg_attn_masked, omg_layernorm and omg_gemm,
// for gfx950.  Contracts: include/omg_hip.h.
//   omg_gemm_skinny     C[M, N] = epi(A[M, K] W[N, K]^T + bias) for few rows: a caption is 6 to 30 tokens, so every Linear is a stream
//                       of its weight against one or two MFMA row blocks.  A workgroup owns 8 or 16 columns of N over the WHOLE of K
//                       (grid.x = N / slice: 96 to 192 workgroups for BERT-base, each streaming its own rows of W exactly once), its
//                       four waves take the 64-wide K steps s = wave, wave + 4, ... and fold their fp32 partial tiles through LDS in
//                       ascending wave order.  Nothing crosses a workgroup: no atomics, no workspace, no second launch.
//   omg_bert_embed_ln   LayerNorm(word[id] + token_type[type] + position[pos]) per token, one wave per token, the row in registers.
#include "common.h"
#include <type_traits>

namespace {

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

constexpr int SK_WAVES = 4;        // K is split over the workgroup's waves
constexpr int SK_STEP = 64;        // K elements per wave step: two 16x16x32 MFMAs
constexpr int SK_ROWS = 16;        // rows of A per MFMA row block

struct SkinnyP {
  int M, N, K, slice;
  const char* A; long lda;
  const char* W; long ldw;
  const char* bias;
  const char* res; long ldr;
  char* C; long ldc;
  int gelu;
};

// The MFMA sums over its 32 k positions; WHICH k a lane's 8 elements are is free as long as both operands agree.  Lane group g = lane >> 4
// takes the 16 consecutive elements k0 + 16 g .. + 15 of a step (32 contiguous bytes per lane, 128 contiguous bytes per row and step),
// the first 8 go to the step's first MFMA and the last 8 to its second.  W is the MFMA's A operand (row = column n of C), the
// activations its B operand (column = row m of C): the result has m on the lane and four consecutive n in its registers, so a lane
// stores 8 contiguous bytes, and row m of C is computed from row m of A alone — MFMA columns never mix.
// Every load is unconditional and branch-free: a chunk beyond K is read from the row's last chunk, a row beyond the slice, N or M from the
// last row inside, and replaced by zeros in registers — the clamp is in the address computation, no byte outside an operand is ever read.
template <typename T, int MB>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(SkinnyP p) {
  using v8 = typename Vec<T>::v8;
  __shared__ f32x4 part[SK_WAVES][MB][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // uniform: the K loop's trip count is scalar
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * p.slice;
  const int m0 = blockIdx.y * (MB * SK_ROWS);
  const int n = n0 + r16;
  const uint32_t n_keep = r16 < p.slice && n < p.N ? ~0u : 0u;
  const int n_last = (n0 + p.slice < p.N ? n0 + p.slice : p.N) - 1;        // the slice's last row: lanes beyond it re-read it (no traffic of their own)
  const char* wrow = p.W + (long)(n < n_last ? n : n_last) * p.ldw * 2;
  const char* arow[MB];
  uint32_t m_keep[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    const int m = m0 + b * SK_ROWS + r16;
    m_keep[b] = m < p.M ? ~0u : 0u;
    arow[b] = p.A + (long)(m < p.M ? m : p.M - 1) * p.lda * 2;
  }
  f32x4 acc[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int steps = (p.K + SK_STEP - 1) / SK_STEP;
  // U steps at once: all 2 U (1 + MB) loads are issued before the first MFMA waits (left to the compiler the loop stays one step deep)
  auto run = [&](int i0, auto u_tag) {
    constexpr int U = decltype(u_tag)::value;
    u32x4 w0[U], w1[U], a0[U][MB], a1[U][MB];
    uint32_t q0[U], q1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = (wave + (i0 + u) * SK_WAVES) * SK_STEP + g * 16;
      const bool k0_ok = k < p.K, k1_ok = k + 8 < p.K;
      const long o0 = (long)(k0_ok ? k : p.K - 8) * 2, o1 = (long)(k1_ok ? k + 8 : p.K - 8) * 2;
      q0[u] = k0_ok ? ~0u : 0u; q1[u] = k1_ok ? ~0u : 0u;
      w0[u] = *(const u32x4*)(wrow + o0); w1[u] = *(const u32x4*)(wrow + o1);
#pragma unroll
      for (int b = 0; b < MB; ++b) { a0[u][b] = *(const u32x4*)(arow[b] + o0); a1[u][b] = *(const u32x4*)(arow[b] + o1); }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // zeros by AND with an all-ones / all-zeros word: a select here is turned back into a branch around the load
      w0[u] &= n_keep & q0[u];
      w1[u] &= n_keep & q1[u];
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        a0[u][b] &= m_keep[b] & q0[u];
        a1[u][b] &= m_keep[b] & q1[u];
        acc[b] = Vec<T>::mfma16(__builtin_bit_cast(v8, w0[u]), __builtin_bit_cast(v8, a0[u][b]), acc[b]);
        acc[b] = Vec<T>::mfma16(__builtin_bit_cast(v8, w1[u]), __builtin_bit_cast(v8, a1[u][b]), acc[b]);
      }
    }
  };
  // steps wave, wave + 4, ... in ascending order: the split and the order are functions of K alone
  const int mine = (steps - wave + SK_WAVES - 1) / SK_WAVES;
  constexpr int UMAX = MB == 4 ? 2 : 4;
  int i = 0;
  for (; i + UMAX <= mine; i += UMAX) run(i, std::integral_constant<int, UMAX>{});
  if (UMAX == 4 && i + 2 <= mine) { run(i, std::integral_constant<int, 2>{}); i += 2; }
  if (i < mine) run(i, std::integral_constant<int, 1>{});
#pragma unroll
  for (int b = 0; b < MB; ++b) part[wave][b][lane] = acc[b];
  __syncthreads();
  // the fold and the epilogue: row block b by wave b mod 4, partials added in ascending wave order (a wave without a step adds zeros)
  for (int b = wave; b < MB; b += SK_WAVES) {
    const int m = m0 + b * SK_ROWS + r16;
    const int nn = n0 + g * 4;
    if (m >= p.M || g * 4 >= p.slice || nn >= p.N) continue;
    f32x4 v = part[0][b][lane];
#pragma unroll
    for (int w = 1; w < SK_WAVES; ++w) v += part[w][b][lane];
    if (p.bias) {
      const typename Vec<T>::v4 bv = *(const typename Vec<T>::v4*)(p.bias + (long)nn * 2);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += (float)bv[e];
    }
    if (p.gelu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = gelu_f(v[e]);
    }
    if (p.res) {
      const typename Vec<T>::v4 rv = *(const typename Vec<T>::v4*)(p.res + ((long)m * p.ldr + nn) * 2);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
    }
    typename Vec<T>::v4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
    *(typename Vec<T>::v4*)(p.C + ((long)m * p.ldc + nn) * 2) = o;
  }
}

// One wave per token; the three rows are summed as (word + type) + position in fp32 and stay in registers for the two-pass statistics
// (ln_kernel of norm.hip).  An id is clamped into its table in the address computation itself.
OMG_DEV long clamp_id(long id, int rows) { return id < 0 ? 0 : (id >= rows ? rows - 1 : id); }

template <typename T, int NV>
__global__ __launch_bounds__(256) void bert_embed_ln_kernel(const long* ids, const long* types, const long* poss, int M, int C,
                                                            const char* word, int n_word, const char* type, int n_type,
                                                            const char* pos, int n_pos, const char* gamma, const char* beta,
                                                            float eps, char* Y, long ldy) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  if (row >= M) return;
  const int nvec = C >> 3;
  const char* wr = word + clamp_id(ids[row], n_word) * C * 2;
  const char* tr = type + clamp_id(types[row], n_type) * C * 2;
  const char* pr = pos + clamp_id(poss[row], n_pos) * C * 2;
  float x[NV][8];
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int vec = lane + v * 64;
    if (vec < nvec) {
      float a[8], b[8], c[8];
      unpack8<T>(*(const u32x4*)(wr + (long)vec * 16), a);
      unpack8<T>(*(const u32x4*)(tr + (long)vec * 16), b);
      unpack8<T>(*(const u32x4*)(pr + (long)vec * 16), c);
#pragma unroll
      for (int e = 0; e < 8; ++e) { x[v][e] = (a[e] + b[e]) + c[e]; s += x[v][e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[v][e] = 0.f;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int vec = lane + v * 64;
    if (vec < nvec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = x[v][e] - mean; q += d * d; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
  const float rstd = rsqrtf(q / (float)C + eps);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int vec = lane + v * 64;
    if (vec < nvec) {
      float ga[8], be[8], y[8];
      unpack8<T>(*(const u32x4*)(gamma + (long)vec * 16), ga);
      unpack8<T>(*(const u32x4*)(beta + (long)vec * 16), be);
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = (x[v][e] - mean) * rstd * ga[e] + be[e];
      *(u32x4*)(Y + ((long)row * ldy + vec * 8) * 2) = pack8<T>(y);
    }
  }
}

}  // namespace

extern "C" int omg_gemm_skinny(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* W, int64_t ldw,
                               const void* bias, int gelu, const void* residual, int64_t ldr, void* C, int64_t ldc, void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_gemm_skinny: dtype");
  OMG_REQUIRE(A && W && C, "omg_gemm_skinny: null operand");
  OMG_REQUIRE(M >= 1 && N >= 1 && K >= 1, "omg_gemm_skinny: M, N, K >= 1");
  OMG_REQUIRE(K % 8 == 0 && N % 8 == 0, "omg_gemm_skinny: K and N multiples of 8");
  OMG_REQUIRE(lda >= K && ldw >= K && ldc >= N && (!residual || ldr >= N), "omg_gemm_skinny: a row stride shorter than its row");
  OMG_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && ldc % 8 == 0 && (!residual || ldr % 8 == 0), "omg_gemm_skinny: row strides multiples of 8");
  OMG_REQUIRE(aligned16(A) && aligned16(W) && aligned16(C) && aligned16(bias) && aligned16(residual), "omg_gemm_skinny: 16-byte aligned operands");
  OMG_REQUIRE(gelu == 0 || gelu == 1, "omg_gemm_skinny: gelu 0 (none) or 1 (erf GELU)");
  SkinnyP p{};
  p.M = M; p.N = N; p.K = K;
  p.slice = N < 2048 ? 8 : 16;           // a function of N alone; the bits of C do not depend on it (every element is its own sum)
  p.A = (const char*)A; p.lda = lda; p.W = (const char*)W; p.ldw = ldw;
  p.bias = (const char*)bias; p.res = (const char*)residual; p.ldr = ldr; p.C = (char*)C; p.ldc = ldc; p.gelu = gelu;
  const int mb = M <= 16 ? 1 : (M <= 32 ? 2 : 4);              // row blocks per workgroup; further rows are grid.y (weights from L2)
  const long gy = ((long)M + mb * SK_ROWS - 1) / (mb * SK_ROWS);
  OMG_REQUIRE(gy <= 65535, "omg_gemm_skinny: grid limits (M <= 64 * 65535)");
  dim3 grid((N + p.slice - 1) / p.slice, (unsigned)gy);
  hipStream_t s = (hipStream_t)stream;
#define SK_LAUNCH(TT) do { \
    if (mb == 1) OMG_LAUNCH((gemm_skinny_kernel<TT, 1>), grid, dim3(256), 0, s, p); \
    else if (mb == 2) OMG_LAUNCH((gemm_skinny_kernel<TT, 2>), grid, dim3(256), 0, s, p); \
    else OMG_LAUNCH((gemm_skinny_kernel<TT, 4>), grid, dim3(256), 0, s, p); } while (0)
  if (dtype == OMG_F16) SK_LAUNCH(f16); else SK_LAUNCH(bf16);
#undef SK_LAUNCH
  return omg_check_launch("gemm_skinny");
}

extern "C" int omg_bert_embed_ln(int dtype, int M, int C, const int64_t* input_ids, const int64_t* token_type_ids,
                                 const int64_t* position_ids, const void* word, int n_word, const void* type, int n_type,
                                 const void* pos, int n_pos, const void* gamma, const void* beta, float eps, void* Y, int64_t ldy,
                                 void* stream) {
  OMG_REQUIRE(dtype == OMG_F16 || dtype == OMG_BF16, "omg_bert_embed_ln: dtype");
  OMG_REQUIRE(input_ids && token_type_ids && position_ids && word && type && pos && gamma && beta && Y, "omg_bert_embed_ln: null operand");
  OMG_REQUIRE(M >= 0 && C >= 8 && C % 8 == 0 && C <= 4096, "omg_bert_embed_ln: width a multiple of 8, at most 4096");
  OMG_REQUIRE(n_word >= 1 && n_type >= 1 && n_pos >= 1, "omg_bert_embed_ln: empty table");
  OMG_REQUIRE(ldy >= C && ldy % 8 == 0, "omg_bert_embed_ln: ldy >= C, a multiple of 8");
  OMG_REQUIRE(aligned16(word) && aligned16(type) && aligned16(pos) && aligned16(gamma) && aligned16(beta) && aligned16(Y),
              "omg_bert_embed_ln: 16-byte aligned operands");
  OMG_REQUIRE((uintptr_t)input_ids % 8 == 0 && (uintptr_t)token_type_ids % 8 == 0 && (uintptr_t)position_ids % 8 == 0,
              "omg_bert_embed_ln: 8-byte aligned ids");
  if (M == 0) return OMG_OK;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((M + 3) / 4);
  const int nv = (C / 8 + 63) / 64;
#define EL_LAUNCH(TT, NVV) OMG_LAUNCH((bert_embed_ln_kernel<TT, NVV>), grid, dim3(256), 0, s, (const long*)input_ids, (const long*)token_type_ids, \
    (const long*)position_ids, M, C, (const char*)word, n_word, (const char*)type, n_type, (const char*)pos, n_pos, (const char*)gamma, \
    (const char*)beta, eps, (char*)Y, (long)ldy)
#define EL_SWITCH(TT) do { if (nv <= 1) EL_LAUNCH(TT, 1); else if (nv <= 2) EL_LAUNCH(TT, 2); else if (nv <= 4) EL_LAUNCH(TT, 4); else EL_LAUNCH(TT, 8); } while (0)
  if (dtype == OMG_F16) EL_SWITCH(f16); else EL_SWITCH(bf16);
#undef EL_SWITCH
#undef EL_LAUNCH
  return omg_check_launch("bert_embed_ln");
}
