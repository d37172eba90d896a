// image_prep.hip — Pillow's 8-bit two-pass resize on precomputed tables, with a preprocessor's normalise / pad / permute / cast in
// the second pass's epilogue, for gfx950 (omg_amd/image_prep.py).  Contracts: include/omg_hip.h.
//   omg_image_resize_h   uint8 [B, H, W, 3] -> uint8 [B, H, OW, 3].  A workgroup is four rows by 64 output pixels; a wave stages the
//                        bytes its row's 64 windows span (one contiguous segment) in LDS through aligned dword loads and every lane
//                        runs its own taps from there.  A segment beyond the LDS buffer (a reduction of a very wide row) or an input
//                        that is not dword aligned is read from global memory by the same loop: same integers, same bits.
//   omg_image_resize_v   the vertical pass, lanes along x: a wave's tap is one contiguous run of 192 bytes, the window and the
//                        coefficients are wave-uniform.  The 8-bit result is stored as it is (uint8 HWC) or looked up in a [3, 256]
//                        table held in LDS and stored planar, with the zeros of the right and bottom pad written by the same launch.
// Both are bound by launch and memory latency (a 1024 x 1024 image is 3 MB): no per-lane arrays, no atomics, run-time tap counts.
#include "common.h"
#include <type_traits>

namespace {

constexpr int IP_BITS = 22;                 // Pillow's PRECISION_BITS for 8-bit pixels
constexpr int IP_TX = 64;                   // output pixels of a workgroup along x: one per lane
constexpr int IP_ROWS = 4;                  // rows of a workgroup: one per wave
constexpr int IP_SEG_DWORDS = 1024;         // LDS bytes / 4 a row's staged segment may take

OMG_DEV int clip8(int ss) {
  const int v = ss >> IP_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct ResizeHP {
  int rows, W, OW, ksize, aligned;          // rows = B H
  long total;                               // bytes of the input
  const uint8_t* in;
  const int* bounds;
  const int* coeffs;
  uint8_t* out;
};

__global__ __launch_bounds__(256) void image_resize_h_kernel(ResizeHP p) {
  __shared__ uint32_t seg[IP_ROWS][IP_SEG_DWORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ox0 = blockIdx.x * IP_TX;
  const int ox_last = (ox0 + IP_TX <= p.OW ? ox0 + IP_TX : p.OW) - 1;
  const long row = (long)blockIdx.y * IP_ROWS + wave;
  // the tile's segment [s0, s1) of input pixels: windows start and end in ascending order, every value is clamped into the row
  int s0 = p.bounds[2 * ox0], s1 = p.bounds[2 * ox_last] + p.bounds[2 * ox_last + 1];
  s0 = s0 < 0 ? 0 : (s0 > p.W ? p.W : s0);
  s1 = s1 < s0 ? s0 : (s1 > p.W ? p.W : s1);
  const long gb = (row * p.W + s0) * 3;                      // first byte of the segment
  const long ga = gb & ~3L;
  const int ndw = (int)((gb + (long)(s1 - s0) * 3 - ga + 3) >> 2);
  const bool use_lds = p.aligned && ndw <= IP_SEG_DWORDS;    // per wave: a wave stages and reads its own row
  if (use_lds && row < p.rows) {
    for (int d = lane; d < ndw; d += 64) {
      const long a = ga + 4L * d;
      uint32_t v;
      if (a + 4 <= p.total) {
        v = *(const uint32_t*)(p.in + a);
      } else {                                               // the input's last, partial dword: byte by byte, nothing behind the tensor
        v = 0;
        for (int b = 0; b < 4; ++b)
          if (a + b < p.total) v |= (uint32_t)p.in[a + b] << (8 * b);
      }
      seg[wave][d] = v;
    }
  }
  __syncthreads();
  const int ox = ox0 + lane;
  if (row >= p.rows || ox >= p.OW) return;
  int xmin = p.bounds[2 * ox], n = p.bounds[2 * ox + 1];
  xmin = xmin < s0 ? s0 : xmin;
  n = n > p.ksize ? p.ksize : n;
  n = xmin + n > s1 ? s1 - xmin : n;                         // no-ops on tables of resize_tables; no tap outside the segment otherwise
  const int* k = p.coeffs + (long)ox * p.ksize;
  int a0 = 1 << (IP_BITS - 1), a1 = a0, a2 = a0;
  if (use_lds) {
    const uint8_t* src = (const uint8_t*)seg[wave] + (int)(gb - ga) + (xmin - s0) * 3;
    for (int t = 0; t < n; ++t) {
      const int c = k[t];
      a0 += (int)src[3 * t] * c; a1 += (int)src[3 * t + 1] * c; a2 += (int)src[3 * t + 2] * c;
    }
  } else {
    const uint8_t* src = p.in + (row * p.W + xmin) * 3;
    for (int t = 0; t < n; ++t) {
      const int c = k[t];
      a0 += (int)src[3 * t] * c; a1 += (int)src[3 * t + 1] * c; a2 += (int)src[3 * t + 2] * c;
    }
  }
  uint8_t* o = p.out + (row * p.OW + ox) * 3;
  o[0] = (uint8_t)clip8(a0); o[1] = (uint8_t)clip8(a1); o[2] = (uint8_t)clip8(a2);
}

struct ResizeVP {
  int H, W, OH, ksize;                      // input [B, H, W, 3]; the result is OH x W
  int Hpad, Wpad;                           // planar output only: [B, 3, Hpad, Wpad]
  const uint8_t* in;
  const int* bounds;                        // NULL: OH == H and the pass is the identity
  const int* coeffs;
  const void* lut;                          // [3, 256] of the output's element, planar output
  void* out;
};

// E = void: uint8 HWC; uint16_t: fp16 / bf16 (bit patterns of the table are copied); uint32_t: fp32
template <typename E>
__global__ __launch_bounds__(256) void image_resize_v_kernel(ResizeVP p) {
  constexpr bool planar = !std::is_void<E>::value;
  using Elem = typename std::conditional<planar, E, uint8_t>::type;
  __shared__ Elem lut[planar ? 768 : 1];
  if (planar) {
    for (int i = threadIdx.x; i < 768; i += 256) lut[i] = ((const Elem*)p.lut)[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x = blockIdx.x * IP_TX + lane;
  const int y = blockIdx.y * IP_ROWS + wave;
  const long b = blockIdx.z;
  const int Hc = planar ? p.Hpad : p.OH, Wc = planar ? p.Wpad : p.W;
  if (y >= Hc || x >= Wc) return;
  int v0 = 0, v1 = 0, v2 = 0;
  const bool inside = y < p.OH && x < p.W;
  if (inside) {
    if (p.bounds) {
      int ymin = p.bounds[2 * y], n = p.bounds[2 * y + 1];
      ymin = ymin < 0 ? 0 : (ymin > p.H ? p.H : ymin);
      n = n > p.ksize ? p.ksize : n;
      n = ymin + n > p.H ? p.H - ymin : n;                   // no-ops on tables of resize_tables; no tap outside the image otherwise
      const int* k = p.coeffs + (long)y * p.ksize;
      const uint8_t* src = p.in + ((b * p.H + ymin) * p.W + x) * 3;
      const long pitch = (long)p.W * 3;
      int a0 = 1 << (IP_BITS - 1), a1 = a0, a2 = a0;
      for (int t = 0; t < n; ++t) {
        const int c = k[t];
        a0 += (int)src[0] * c; a1 += (int)src[1] * c; a2 += (int)src[2] * c;
        src += pitch;
      }
      v0 = clip8(a0); v1 = clip8(a1); v2 = clip8(a2);
    } else {
      const uint8_t* src = p.in + ((b * p.H + y) * p.W + x) * 3;
      v0 = src[0]; v1 = src[1]; v2 = src[2];
    }
  }
  if constexpr (planar) {
    const long plane = (long)p.Hpad * p.Wpad;
    Elem* o = (Elem*)p.out + b * 3 * plane + (long)y * p.Wpad + x;
    o[0] = inside ? lut[v0] : (Elem)0;
    o[plane] = inside ? lut[256 + v1] : (Elem)0;
    o[2 * plane] = inside ? lut[512 + v2] : (Elem)0;
  } else {
    uint8_t* o = (uint8_t*)p.out + ((b * p.OH + y) * p.W + x) * 3;
    o[0] = (uint8_t)v0; o[1] = (uint8_t)v1; o[2] = (uint8_t)v2;
  }
}

bool sizes_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && (long)B * H * W * 3 < (1L << 40); }

}  // namespace

extern "C" int omg_image_resize_h(int B, int H, int W, int OW, const uint8_t* in, const int32_t* bounds, const int32_t* coeffs, int ksize,
                                  uint8_t* out, void* stream) {
  OMG_REQUIRE(in && bounds && coeffs && out, "omg_image_resize_h: null operand");
  OMG_REQUIRE(sizes_ok(B, H, W) && OW >= 1 && sizes_ok(B, H, OW), "omg_image_resize_h: B, H, W, OW >= 1");
  OMG_REQUIRE(ksize >= 1, "omg_image_resize_h: ksize >= 1");
  OMG_REQUIRE((uintptr_t)bounds % 4 == 0 && (uintptr_t)coeffs % 4 == 0, "omg_image_resize_h: 4-byte aligned tables");
  const long rows = (long)B * H;
  const long gy = (rows + IP_ROWS - 1) / IP_ROWS;
  ResizeHP p{};
  p.rows = (int)rows; p.W = W; p.OW = OW; p.ksize = ksize; p.aligned = (uintptr_t)in % 4 == 0;
  p.total = rows * W * 3;
  p.in = in; p.bounds = bounds; p.coeffs = coeffs; p.out = out;
  dim3 grid((OW + IP_TX - 1) / IP_TX, (unsigned)gy);
  OMG_REQUIRE(gy <= 65535, "omg_image_resize_h: B H at most 4 * 65535 rows");
  OMG_LAUNCH(image_resize_h_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
  return omg_check_launch("image_resize_h");
}

extern "C" int omg_image_resize_v(int B, int H, int W, int OH, const uint8_t* in, const int32_t* bounds, const int32_t* coeffs, int ksize,
                                  int out_dtype, const void* lut, int Hpad, int Wpad, void* out, void* stream) {
  OMG_REQUIRE(in && out, "omg_image_resize_v: null operand");
  OMG_REQUIRE(sizes_ok(B, H, W) && OH >= 1 && sizes_ok(B, OH, W), "omg_image_resize_v: B, H, W, OH >= 1");
  if (bounds) {
    OMG_REQUIRE(coeffs && ksize >= 1, "omg_image_resize_v: bounds without coefficients");
    OMG_REQUIRE((uintptr_t)bounds % 4 == 0 && (uintptr_t)coeffs % 4 == 0, "omg_image_resize_v: 4-byte aligned tables");
  } else {
    OMG_REQUIRE(OH == H, "omg_image_resize_v: no tables (the identity pass) needs OH == H");
  }
  OMG_REQUIRE(B <= 65535, "omg_image_resize_v: B at most 65535");
  ResizeVP p{};
  p.H = H; p.W = W; p.OH = OH; p.ksize = ksize; p.in = in; p.bounds = bounds; p.coeffs = coeffs; p.lut = lut; p.out = out;
  hipStream_t s = (hipStream_t)stream;
  if (!lut) {
    p.Hpad = OH; p.Wpad = W;
    OMG_REQUIRE((OH + IP_ROWS - 1) / IP_ROWS <= 65535, "omg_image_resize_v: OH at most 4 * 65535");
    dim3 grid((W + IP_TX - 1) / IP_TX, (OH + IP_ROWS - 1) / IP_ROWS, B);
    OMG_LAUNCH(image_resize_v_kernel<void>, grid, dim3(256), 0, s, p);
    return omg_check_launch("image_resize_v");
  }
  OMG_REQUIRE(out_dtype == OMG_F16 || out_dtype == OMG_BF16 || out_dtype == OMG_F32, "omg_image_resize_v: out_dtype of the planar output");
  OMG_REQUIRE(Hpad >= OH && Wpad >= W && sizes_ok(B, Hpad, Wpad), "omg_image_resize_v: the pad is at the right and bottom (Hpad >= OH, Wpad >= W)");
  OMG_REQUIRE((Hpad + IP_ROWS - 1) / IP_ROWS <= 65535, "omg_image_resize_v: Hpad at most 4 * 65535");
  OMG_REQUIRE((uintptr_t)lut % 4 == 0 && (uintptr_t)out % 4 == 0, "omg_image_resize_v: 4-byte aligned table and output");
  p.Hpad = Hpad; p.Wpad = Wpad;
  dim3 grid((Wpad + IP_TX - 1) / IP_TX, (Hpad + IP_ROWS - 1) / IP_ROWS, B);
  if (out_dtype == OMG_F32) OMG_LAUNCH(image_resize_v_kernel<uint32_t>, grid, dim3(256), 0, s, p);
  else OMG_LAUNCH(image_resize_v_kernel<uint16_t>, grid, dim3(256), 0, s, p);
  return omg_check_launch("image_resize_v");
}
