// p2p_vmap.hip — the general prompt-to-prompt cross-attention edit folded into V, for gfx950.
// Reference: src/prompt_attention/p2p_attention.py:131-133, :147 (AttentionReplace.replace_cross_attention + the alpha blend).
//
// For an edited sample e with base sample b the reference forms, per head and query row,
//     P_new = (P_b M_e) * alpha_e + (1 - alpha_e) * P_e         (alpha per key n)
//     O_e   = P_new V_e  =  P_b V'_e + P_e V''_e
//     V'_e[w, :]  = sum_n M_e[w, n] alpha_e[n] V_e[n, :]          V''_e[n, :] = (1 - alpha_e[n]) V_e[n, :]
// so the edit is two launches of the unchanged flash kernel (Q, K borrowed from b on V'; own Q, K accumulating on V'') once the two
// V^T images exist.  omg_transpose_v_mapped writes both for the whole batch in one launch, in omg_transpose_v's MFMA key order with
// zero-padded columns; rows that are not edited get the plain transpose and a zero second image.
//
// One workgroup per (64 output keys, head, sample): the sample's V slice (<= 128 keys x 64) and the 64 x Nkv block of
// M_e diag(alpha_e) are staged once in LDS, every thread owns one d and 16 output keys, fp32 accumulation over n, one rounding.
// A coefficient that is exactly 0 is skipped, not multiplied: a non-finite V row behind it never reaches the output.
// About 0.8 MFLOP per (sample, head): plain VALU, launch-bound.
#include "common.h"

namespace {

struct VMapP {
  const char* V; long ldv, v_bs;
  int heads, Nkv, Nkv_pad, E, steps;
  const int* edit_of;
  const float* mapper; long ld_m, m_es;
  const float* alpha; long a_ss, a_es;
  const int* step_idx;
  char* Vm; char* Vo;
};

constexpr int VM_KEYS = 128;      // Nkv <= 128: the resident-K/V attention kernel's limit

// tile[64 keys][64 d] -> 64 columns kv0.. of Vt rows (b, h, d), keys of every 16 in the order [0-3, 8-11 | 4-7, 12-15] (transpose_v_kernel)
template <typename T>
OMG_DEV void vmap_store_tile(const T (&tile)[64][66], char* Vt, long row0, int Nkv_pad, int kv0, int tid) {
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int d = ps * 32 + (tid >> 3), c = tid & 7;
    const int kb = (c >> 1) * 16 + (c & 1) * 4;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)tile[kb + (e & 3) + (e >> 2) * 8][d];
    *(u32x4*)(Vt + ((row0 + d) * Nkv_pad + kv0 + c * 8) * 2) = pack8<T>(f);
  }
}

// grid (Nkv_pad / 64, heads, B)
template <typename T>
__global__ __launch_bounds__(256) void transpose_v_mapped_kernel(VMapP p) {
  __shared__ float Cs[64 * VM_KEYS];          // M_e[kv0 + w][n] * alpha_e[n]
  __shared__ float As[VM_KEYS];               // 1 - alpha_e[n]
  __shared__ T Vs[VM_KEYS][66];               // the sample's V slice of this head, rows >= Nkv zero
  __shared__ T tile[64][66];
  const int tid = threadIdx.x;
  const int kv0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  int e = p.edit_of[b];
  if (e >= p.E) e = p.E - 1;                  // a table index read from the device is clamped, never trusted
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int key = ps * 32 + (tid >> 3), c = tid & 7;
    float f[8];
    if (key < p.Nkv) {
      unpack8<T>(*(const u32x4*)(p.V + ((long)b * p.v_bs + (long)key * p.ldv + h * 64 + c * 8) * 2), f);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) Vs[key][c * 8 + i] = (T)f[i];
  }
  if (e >= 0) {
    int step = p.step_idx != nullptr ? *p.step_idx : 0;
    step = step < 0 ? 0 : (step >= p.steps ? p.steps - 1 : step);
    const float* al = p.alpha + (long)step * p.a_ss + (long)e * p.a_es;
    const float* M = p.mapper + (long)e * p.m_es;
    for (int idx = tid; idx < 64 * VM_KEYS; idx += 256) {
      const int n = idx & (VM_KEYS - 1), w = kv0 + (idx >> 7);
      Cs[idx] = (w < p.Nkv && n < p.Nkv) ? M[(long)w * p.ld_m + n] * al[n] : 0.f;
    }
    if (tid < VM_KEYS) As[tid] = tid < p.Nkv ? 1.f - al[tid] : 0.f;
  }
  __syncthreads();
  const int d = tid & 63, w0 = (tid >> 6) * 16;
  float acc[16];
  if (e >= 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int n = 0; n < p.Nkv; ++n) {
      const float v = (float)Vs[n][d];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float c = Cs[(w0 + i) * VM_KEYS + n];
        acc[i] = c != 0.f ? fmaf(c, v, acc[i]) : acc[i];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = kv0 + w0 + i < VM_KEYS ? (float)Vs[kv0 + w0 + i][d] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[w0 + i][d] = (T)acc[i];
  __syncthreads();
  const long row0 = (long)(b * p.heads + h) * 64;
  vmap_store_tile<T>(tile, p.Vm, row0, p.Nkv_pad, kv0, tid);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int n = kv0 + w0 + i;
    float r = 0.f;
    if (e >= 0 && n < VM_KEYS) {
      const float c = As[n];
      r = c != 0.f ? c * (float)Vs[n][d] : 0.f;
    }
    tile[w0 + i][d] = (T)r;
  }
  __syncthreads();
  vmap_store_tile<T>(tile, p.Vo, row0, p.Nkv_pad, kv0, tid);
}

}  // namespace

extern "C" int omg_transpose_v_mapped(const omg_vmap_args* a, void* stream) {
  OMG_REQUIRE(a != nullptr, "omg_transpose_v_mapped: null args");
  OMG_REQUIRE(a->dtype == OMG_F16 || a->dtype == OMG_BF16, "omg_transpose_v_mapped: dtype");
  OMG_REQUIRE(a->B > 0 && a->heads > 0 && a->Nkv > 0, "omg_transpose_v_mapped: shape");
  OMG_REQUIRE(a->Nkv <= VM_KEYS, "omg_transpose_v_mapped: at most 128 keys (the edit exists for cross-attention only)");
  OMG_REQUIRE(a->Nkv_pad % 64 == 0 && a->Nkv_pad >= a->Nkv, "omg_transpose_v_mapped: Nkv_pad");
  OMG_REQUIRE(a->E > 0 && a->steps > 0, "omg_transpose_v_mapped: E and steps must be positive");
  OMG_REQUIRE(a->V && a->edit_of && a->mapper && a->alpha && a->Vt_mapped && a->Vt_own, "omg_transpose_v_mapped: null operand");
  OMG_REQUIRE(a->ldv % 8 == 0 && a->v_bstride % 8 == 0 && ((uintptr_t)a->V & 15) == 0,
              "omg_transpose_v_mapped: V must be 16-byte aligned with ldv and v_bstride multiples of 8 elements");
  OMG_REQUIRE(((uintptr_t)a->Vt_mapped & 15) == 0 && ((uintptr_t)a->Vt_own & 15) == 0, "omg_transpose_v_mapped: outputs must be 16-byte aligned");
  OMG_REQUIRE(a->ld_mapper >= a->Nkv && a->mapper_estride >= 0 && a->alpha_step_stride >= 0 && a->alpha_estride >= 0,
              "omg_transpose_v_mapped: table strides");
  VMapP p{};
  p.V = (const char*)a->V; p.ldv = a->ldv; p.v_bs = a->v_bstride;
  p.heads = a->heads; p.Nkv = a->Nkv; p.Nkv_pad = a->Nkv_pad; p.E = a->E; p.steps = a->steps;
  p.edit_of = a->edit_of;
  p.mapper = a->mapper; p.ld_m = a->ld_mapper; p.m_es = a->mapper_estride;
  p.alpha = a->alpha; p.a_ss = a->alpha_step_stride; p.a_es = a->alpha_estride;
  p.step_idx = a->step_idx;
  p.Vm = (char*)a->Vt_mapped; p.Vo = (char*)a->Vt_own;
  dim3 grid(a->Nkv_pad / 64, a->heads, a->B);
  hipStream_t s = (hipStream_t)stream;
  if (a->dtype == OMG_F16) OMG_LAUNCH(transpose_v_mapped_kernel<f16>, grid, dim3(256), 0, s, p);
  else OMG_LAUNCH(transpose_v_mapped_kernel<bf16>, grid, dim3(256), 0, s, p);
  return omg_check_launch("transpose_v_mapped");
}
