// conv_f32_wino.hip — fp32 3x3 / stride 1 / pad 1 convolution as Winograd F(2x2, 3x3) on the f32-input MFMA for gfx950.
//
// The direct kernel (gemm_f32.hip) spends 36 multiplies per 2x2 output tile and input channel; F(2x2, 3x3) spends 16:
//
//   Y(2x2) = A^T [ sum_cin (G g G^T) .* (B^T d B) ] A          d: 4x4 input patch, g: 3x3 filter
//
// i.e. 16 independent GEMMs M_pos[tile][cout] = V_pos[tile][cin] . U_pos[cout][cin]^T, one per transform position.  U = G g G^T is
// built once per weight on the host side (ops.pack_conv_weight_wino) in exactly the order the kernel streams it.
//
// A workgroup owns an 8 x 8 patch of tiles (16 x 16 output pixels of one image) x 64 output channels x all 16 positions; each of
// its four waves owns 32 tiles x 32 channels and holds ALL 16 positions of that sub-block (16 x 16 = 256 accumulator registers, one
// wave per SIMD), so the output transform A^T m A is lane-local adds.  K stage = 8 input channels:
//   V stage: the block's raw 18 x 18 pixel patch (32 bytes per pixel) comes in by LDS-DMA, one stage ahead; a lane reads 3 x 4 pixels x
//            16 bytes of its tile from it, applies B^T d B (two waves per tile and channel quad, each computing two of the four
//            transform rows) and writes 8 positions with ds_write_b128 (per-tile global loads instead of the shared patch: 4.7 x the
//            load requests; measured 1.32 x slower on the decode);
//   U stage: 32 KiB contiguous in the weight image, filled by LDS-DMA (8 pieces of 1 KiB per wave);
//   LDS image of both operands: [pos 16][k chunk 2][row 64][16 bytes] — a wave's ds_read_b128 covers 32 consecutive 16-byte slots
//   per lane half (conflict free); the e-th float of the chunk feeds MFMA e (k = 4 h + e, the same map on both operands).
// Both operands and the raw patch are double buffered (4 x 32 KiB + 2 x 12 KiB of LDS).  64 MFMAs x 64 cycles per wave and stage against 32 ds_read_b128.
// The accumulators hold the transposed tile (mfma(U, V)): a lane owns one tile and runs of 4 consecutive channels = 16-byte stores.
// Out-of-image taps are lane offsets beyond the descriptor's range (zeros); the fused nearest-2x upsample reads pixel (y >> 1, x >> 1).
#include "common.h"

namespace {

constexpr int WSTAGE = 16 * 2 * 64 * 16;        // 32 KiB per operand and stage
constexpr int WRAW = 3 * 4096;                  // raw input patch of a stage: 18 x 18 pixels x 32 bytes, rounded up to 3 DMA pieces per wave
constexpr int WLDS = 4 * WSTAGE + 2 * WRAW;     // V0 V1 U0 U1 R0 R1 = 152 KiB
constexpr unsigned WINO_OOB = 0xfff00000u;      // beyond every descriptor of this file: the buffer unit returns zeros

struct WinoP {
  const char* X; const char* U; const char* bias; const char* residual; char* Y;
  int Hin, Win, Cin, Hout, Wout, Cout, upsample;
  int py, px, nb;                               // patches per image (rows, columns), channel blocks
  unsigned u_bytes;
};

typedef __attribute__((address_space(3))) void* wino_lds_ptr_t;

__device__ __forceinline__ void wino_dma16(__amdgpu_buffer_rsrc_t rs, char* lds, unsigned voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (wino_lds_ptr_t)lds, 16, (int)voff, soff, 0, 0);
}

__global__ __launch_bounds__(256, 1) void conv_f32_wino_kernel(WinoP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];      // V0 V1 U0 U1 R0 R1
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int nb = bid % p.nb;                    // channel blocks fastest: consecutive blocks of an XCD share the input patch
  int t = bid / p.nb;
  const int bx = t % p.px; t /= p.px;
  const int by = t % p.py;
  const int b = t / p.py;
  const int Y0 = by * 16, X0 = bx * 16;

  // 32-bit lane offsets from the block's own image, so that inputs beyond 4 GB keep working
  const long img_bytes = (long)p.Hin * p.Win * p.Cin * 4;
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)(p.X + (long)b * img_bytes), 0,
                                                                      (int)(unsigned)(img_bytes < (long)WINO_OOB ? img_bytes : (long)WINO_OOB), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsU = __builtin_amdgcn_make_buffer_rsrc((void*)p.U, 0, (int)p.u_bytes, 0x00020000);

  // the raw 18 x 18 input patch of a stage, [pixel][channel quad] x 16 bytes, by LDS-DMA: slot = 256 i + tid, 3 pieces per wave
  unsigned voffR[3];
  {
    const int Hl = p.upsample ? p.Hin * 2 : p.Hin, Wl = p.upsample ? p.Win * 2 : p.Win;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int s = i * 256 + tid, pixel = s >> 1, quad = s & 1;
      const int pr = pixel / 18;
      int iy = Y0 - 1 + pr, ix = X0 - 1 + (pixel - pr * 18);
      const bool ok = (pixel < 324) & ((unsigned)iy < (unsigned)Hl) & ((unsigned)ix < (unsigned)Wl);
      if (p.upsample) { iy >>= 1; ix >>= 1; }
      voffR[i] = ok ? ((unsigned)(iy * p.Win + ix) * (unsigned)p.Cin + (unsigned)quad * 4u) * 4u : WINO_OOB;
    }
  }
  const int nk = p.Cin >> 3;
  const unsigned voffU = (unsigned)tid * 16u;
  const int ubase = nb * nk;

  auto dma_x = [&](int rbuf, int kt) {
    char* dst = smem + 4 * WSTAGE + rbuf * WRAW + w * 1024;
#pragma unroll
    for (int i = 0; i < 3; ++i) wino_dma16(rsX, dst + i * 4096, voffR[i], kt * 32);
  };
  auto dma_u = [&](int buf, int kt) {
    char* dst = smem + (2 + buf) * WSTAGE + w * 1024;
    const int soff = (ubase + kt) * WSTAGE;
#pragma unroll
    for (int i = 0; i < 8; ++i) wino_dma16(rsU, dst + i * 4096, voffU + i * 4096u, soff);
  };
  // input transform role: tile = lane (8 x 8), channel quad cq, transform rows 2 half, 2 half + 1 (from patch rows half .. half + 2 of the tile):
  // B^T d B -> positions 8 half .. 8 half + 7 of the V image
  const int cq = w & 1, half = w >> 1;
  const int offR = ((2 * (lane >> 3) + half) * 18 + 2 * (lane & 7)) * 32 + cq * 16;
  auto transform = [&](int buf, int rbuf) {
    const char* src = smem + 4 * WSTAGE + rbuf * WRAW + offR;
    f32x4 d0[4], d1[4], d2[4], ta[4], v1[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      d0[c] = *(const f32x4*)(src + c * 32); d1[c] = *(const f32x4*)(src + (18 + c) * 32); d2[c] = *(const f32x4*)(src + (36 + c) * 32);
    }
    // Differences before sums: on inputs with a common offset (post-SiLU activations) a difference of neighbours is exact and small, a
    // sum is large and rounded.  Rows d0 d1 d2: t0 = d0 - d2 and t1 = d1 + d2 — the sum row takes its COLUMN transform first, per row,
    // and adds last (rows first, t1's rounding, relative to 2 |d|, came out of the column differences relative to |V| << |d|).
    // Rows d1 d2 d3 (d0 d1 d2 here): t2 = d2 - d1, t3 = d1 - d3, both differences.
    if (half == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) ta[c] = d0[c] - d2[c];
      v1[0] = (d1[0] - d1[2]) + (d2[0] - d2[2]);
      v1[1] = (d1[1] + d1[2]) + (d2[1] + d2[2]);
      v1[2] = (d1[2] - d1[1]) + (d2[2] - d2[1]);
      v1[3] = (d1[1] - d1[3]) + (d2[1] - d2[3]);
    } else {
      f32x4 tb[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) { ta[c] = d1[c] - d0[c]; tb[c] = d0[c] - d2[c]; }
      v1[0] = tb[0] - tb[2]; v1[1] = tb[1] + tb[2]; v1[2] = tb[2] - tb[1]; v1[3] = tb[1] - tb[3];
    }
    char* dst = smem + buf * WSTAGE + (half * 8 * 2 + cq) * 1024 + lane * 16;
    *(f32x4*)(dst + 0 * 2048) = ta[0] - ta[2];
    *(f32x4*)(dst + 1 * 2048) = ta[1] + ta[2];
    *(f32x4*)(dst + 2 * 2048) = ta[2] - ta[1];
    *(f32x4*)(dst + 3 * 2048) = ta[1] - ta[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) *(f32x4*)(dst + (4 + j) * 2048) = v1[j];
  };

  const int wm = w >> 1, wn = w & 1;
  f32x16 acc[16];                               // acc[pos]: tile wm * 32 + l31, channels wn * 32 + 8 g + 4 hi + {0..3} (g = reg >> 2)
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const int offV = hi * 1024 + (wm * 32 + l31) * 16, offU = hi * 1024 + (wn * 32 + l31) * 16;
  auto mfmas = [&](int buf, int pos) {
    const f32x4 vf = *(const f32x4*)(smem + buf * WSTAGE + pos * 2048 + offV);
    const f32x4 uf = *(const f32x4*)(smem + (2 + buf) * WSTAGE + pos * 2048 + offU);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[pos] = __builtin_amdgcn_mfma_f32_32x32x2f32(uf[e], vf[e], acc[pos], 0, 0, 0);
  };

  // stage kt computes from V[kt & 1], U[kt & 1]; meanwhile U(kt + 1) and the raw patch of stage kt + 2 are in flight and the patch of
  // stage kt + 1 (landed before this stage's barrier) is transformed into V[(kt + 1) & 1] in the shadow of the MFMAs
  dma_x(0, 0);
  dma_u(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  transform(0, 0);
  if (nk > 1) dma_x(1, 1);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) dma_u(buf ^ 1, kt + 1);
    if (kt + 2 < nk) dma_x(buf, kt + 2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pos = 0; pos < 4; ++pos) mfmas(buf, pos);
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nk) transform(buf ^ 1, buf ^ 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pos = 4; pos < 16; ++pos) mfmas(buf, pos);
  }

  // ---- epilogue: A^T m A per register (lane-local), bias + residual, 16-byte stores
  const int tile = wm * 32 + l31;
  const int oy = Y0 + 2 * (tile >> 3), ox = X0 + 2 * (tile & 7);
  if (oy >= p.Hout || ox >= p.Wout) return;     // Hout, Wout even: a 2 x 2 tile is inside or outside as a whole
  const long pix = ((long)b * p.Hout + oy) * p.Wout + ox;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int c = nb * 64 + wn * 32 + g * 8 + hi * 4;
    if (c >= p.Cout) continue;                  // Cout % 4 == 0
    f32x4 y[2][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = g * 4 + q;
      float s0[4], s1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s0[j] = acc[j][r] + acc[4 + j][r] + acc[8 + j][r];
        s1[j] = acc[4 + j][r] - acc[8 + j][r] - acc[12 + j][r];
      }
      y[0][0][q] = s0[0] + s0[1] + s0[2]; y[0][1][q] = s0[1] - s0[2] - s0[3];
      y[1][0][q] = s1[0] + s1[1] + s1[2]; y[1][1][q] = s1[1] - s1[2] - s1[3];
    }
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) bv = *(const f32x4*)(p.bias + (long)c * 4);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const long o = ((pix + (long)a * p.Wout + e) * p.Cout + c) * 4;
        f32x4 v = y[a][e] + bv;
        if (p.residual) v += *(const f32x4*)(p.residual + o);
        *(f32x4*)(p.Y + o) = v;
      }
  }
}

}  // namespace

extern "C" int64_t omg_conv2d_f32_wino_weight_floats(int Cout, int Cin) {
  return (int64_t)((Cout + 63) / 64) * (Cin / 8) * (WSTAGE / 4);
}

extern "C" int omg_conv2d_f32_wino(const omg_conv2d_f32_wino_args* a, void* stream) {
  OMG_REQUIRE(a != nullptr, "omg_conv2d_f32_wino: null args");
  OMG_REQUIRE(a->Cin > 0 && a->Cin % 8 == 0 && a->Cout > 0 && a->Cout % 4 == 0, "omg_conv2d_f32_wino: Cin % 8, Cout % 4");
  OMG_REQUIRE(a->X && a->U && a->Y, "omg_conv2d_f32_wino: null operand");
  const int Hl = a->upsample ? 2 * a->Hin : a->Hin, Wl = a->upsample ? 2 * a->Win : a->Win;
  OMG_REQUIRE(a->Hout == Hl && a->Wout == Wl, "omg_conv2d_f32_wino: 3x3, stride 1, 'same' padding only");
  OMG_REQUIRE(a->Hout % 2 == 0 && a->Wout % 2 == 0, "omg_conv2d_f32_wino: even output sizes only (2x2 tiles)");
  if (a->B == 0 || a->Hout == 0 || a->Wout == 0) return OMG_OK;
  WinoP p{};
  p.X = (const char*)a->X; p.U = (const char*)a->U; p.bias = (const char*)a->bias; p.residual = (const char*)a->residual; p.Y = (char*)a->Y;
  p.Hin = a->Hin; p.Win = a->Win; p.Cin = a->Cin; p.Hout = a->Hout; p.Wout = a->Wout; p.Cout = a->Cout; p.upsample = a->upsample;
  p.py = (a->Hout + 15) / 16; p.px = (a->Wout + 15) / 16; p.nb = (a->Cout + 63) / 64;
  const long img_bytes = (long)a->Hin * a->Win * a->Cin * 4, u_bytes = (long)omg_conv2d_f32_wino_weight_floats(a->Cout, a->Cin) * 4;
  const long blocks = (long)a->B * p.py * p.px * p.nb;
  OMG_REQUIRE(img_bytes < (long)WINO_OOB && u_bytes < 0x7fffffffL && blocks < 0x7fffffffL,
              "omg_conv2d_f32_wino: an image / the weight image beyond the 32-bit offsets of the kernel");
  p.u_bytes = (unsigned)u_bytes;
  static bool attr = false;
  if (!attr) { attr = true; (void)hipFuncSetAttribute((const void*)conv_f32_wino_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WLDS); }
  OMG_LAUNCH(conv_f32_wino_kernel, dim3((unsigned)blocks), dim3(256), WLDS, (hipStream_t)stream, p);
  return omg_check_launch("conv2d_f32_wino");
}
