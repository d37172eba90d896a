// canny.hip — the demos' Canny edge condition (cv2.Canny(image, t1, t2), apertureSize 3, L1 gradient) for gfx950 (omg_amd/canny.py has
// the arithmetic as a numpy model).  Contracts: include/omg_hip.h.  Integers throughout: the result is a function of the input alone.
//   omg_canny_nms         uint8 [B, H, W, C] -> uint8 state [B, H, W] (0 none, 1 weak, 2 strong) in one launch.  A workgroup owns 64 x 16
//                         pixels: it stages the source bytes of the tile and a two-pixel halo in LDS through aligned dword loads (rows
//                         clamped into the image: that is the replicated border), forms the Sobel pair and |dx| + |dy| of the channel
//                         with the largest magnitude for the tile and a one-pixel halo (0 outside the image), and a lane decides four
//                         pixels of a row and stores them as one dword where the address allows it.  Nothing but the source is read
//                         and nothing but the states is written.
//   omg_canny_hysteresis  state -> edges: connected-component labelling by union-find over pixel indices, four launches whatever the data:
//                         (a) canny_label_tile_kernel: labels of a 64 x 16 tile to their fixpoint in LDS, the tile-root index per candidate
//                         (-1 elsewhere) and a zero flag per pixel; (b) canny_border_union_kernel: find / atomicMin union of the pairs that
//                         cross a tile border; (c) canny_flatten_kernel: every label to its root, strong pixels store 1 to their root's
//                         flag; (d) canny_edges_kernel: 255 (or 1.0) where the root's flag is set.  No kernel waits for another workgroup;
//                         the only loops on global memory are the lock-free find / atomicMin retries, which end because a parent is
//                         never above its child.
#include "common.h"
#include <type_traits>

namespace {

constexpr int CN_TW = 64, CN_TH = 16;             // the tile of both tiled kernels
constexpr int CN_MW = CN_TW + 2, CN_MH = CN_TH + 2;   // tile and a one-pixel halo: magnitudes, labels
constexpr int CN_MP = CN_TW + 4;                  // pitch of the 16-bit magnitude rows
constexpr int CN_SH = CN_TH + 4;                  // source rows: a two-pixel halo
constexpr int CN_NONE = 0x7fffffff;               // label of a pixel that is no candidate

template <int C> struct NmsLds {
  static constexpr int SRC_DW = ((CN_TW + 4) * C + 3 + 3) / 4;     // a row's bytes and up to three in front of them, in dwords
  uint32_t src[CN_SH][SRC_DW];
  uint32_t dxdy[CN_TH][CN_TW];                    // dx | dy << 16 of the chosen channel, as two int16
  uint16_t mag[CN_MH][CN_MP];
  int rowoff[CN_SH];                              // bytes between a staged row's first dword and its first pixel
};

struct NmsP {
  int H, W, low, high;
  long total;                                     // bytes of the image
  const uint8_t* in;
  uint8_t* state;
};

template <int C>
__global__ __launch_bounds__(256) void canny_nms_kernel(NmsP p) {
  __shared__ NmsLds<C> s;
  constexpr int SRC_DW = NmsLds<C>::SRC_DW;
  const int tx0 = blockIdx.x * CN_TW, ty0 = blockIdx.y * CN_TH;
  const long b = blockIdx.z;
  const int x_lo = tx0 - 2 < 0 ? 0 : tx0 - 2;
  const int x_hi = tx0 + CN_TW + 1 > p.W - 1 ? p.W - 1 : tx0 + CN_TW + 1;
  const int nbytes = (x_hi - x_lo + 1) * C;
  // stage: row r of the buffer is image row clamp(ty0 - 2 + r), columns x_lo .. x_hi
  for (int idx = threadIdx.x; idx < CN_SH * SRC_DW; idx += 256) {
    const int r = idx / SRC_DW, d = idx - r * SRC_DW;
    int y = ty0 - 2 + r;
    y = y < 0 ? 0 : (y > p.H - 1 ? p.H - 1 : y);
    const long gb = ((b * p.H + y) * p.W + x_lo) * C;            // first byte of the row's segment
    const int off = (int)(((uintptr_t)p.in + (uintptr_t)gb) & 3);
    if (d == 0) s.rowoff[r] = off;
    const long a = gb - off + 4L * d;                            // a dword-aligned address, as an offset into the image
    if (a >= gb + nbytes) continue;
    uint32_t v;
    if (a >= 0 && a + 4 <= p.total) {
      v = *(const uint32_t*)(p.in + a);
    } else {                                                     // the tensor's first or last, partial dword: nothing outside it is read
      v = 0;
      for (int k = 0; k < 4; ++k)
        if (a + k >= 0 && a + k < p.total) v |= (uint32_t)p.in[a + k] << (8 * k);
    }
    s.src[r][d] = v;
  }
  __syncthreads();
  // gradients and magnitudes of the tile and a one-pixel halo
  for (int q = threadIdx.x; q < CN_MH * CN_MW; q += 256) {
    const int i = q / CN_MW, j = q - i * CN_MW;
    const int y = ty0 - 1 + i, x = tx0 - 1 + j;
    int bm = 0, bdx = 0, bdy = 0;
    if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
      const int xl = (x > 0 ? x - 1 : 0) - x_lo, xc = x - x_lo, xr = (x < p.W - 1 ? x + 1 : x) - x_lo;
      const uint8_t* r0 = (const uint8_t*)s.src[i] + s.rowoff[i];
      const uint8_t* r1 = (const uint8_t*)s.src[i + 1] + s.rowoff[i + 1];
      const uint8_t* r2 = (const uint8_t*)s.src[i + 2] + s.rowoff[i + 2];
      bm = -1;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int a00 = r0[xl * C + c], a01 = r0[xc * C + c], a02 = r0[xr * C + c];
        const int a10 = r1[xl * C + c], a12 = r1[xr * C + c];
        const int a20 = r2[xl * C + c], a21 = r2[xc * C + c], a22 = r2[xr * C + c];
        const int dx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
        const int dy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
        const int m = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
        if (m > bm) { bm = m; bdx = dx; bdy = dy; }              // strictly larger: the lowest channel wins a tie
      }
    }
    s.mag[i][j] = (uint16_t)bm;
    if (i >= 1 && i <= CN_TH && j >= 1 && j <= CN_TW) s.dxdy[i - 1][j - 1] = ((uint32_t)bdx & 0xffffu) | ((uint32_t)bdy << 16);
  }
  __syncthreads();
  // non-maximum suppression: a lane takes four pixels of a row
  const int ly = threadIdx.x >> 4, lx = (threadIdx.x & 15) * 4;
  const int y = ty0 + ly, x0 = tx0 + lx;
  if (y >= p.H || x0 >= p.W) return;
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = ly + 1, j = lx + k + 1;
    const int m = s.mag[i][j];
    uint32_t st = 0;
    if (m > p.low) {
      const uint32_t g = s.dxdy[ly][lx + k];
      const int dx = (int16_t)(g & 0xffffu), dy = (int16_t)(g >> 16);
      const int ax = dx < 0 ? -dx : dx, ay = (dy < 0 ? -dy : dy) << 15;
      const int t22 = ax * 13573, t67 = t22 + (ax << 16);
      bool keep;
      if (ay < t22) {
        keep = m > s.mag[i][j - 1] && m >= s.mag[i][j + 1];
      } else if (ay > t67) {
        keep = m > s.mag[i - 1][j] && m >= s.mag[i + 1][j];
      } else {
        const int sg = (dx ^ dy) < 0 ? -1 : 1;
        keep = m > s.mag[i - 1][j - sg] && m > s.mag[i + 1][j + sg];
      }
      st = keep ? (m > p.high ? 2u : 1u) : 0u;
    }
    packed |= st << (8 * k);
  }
  uint8_t* o = p.state + (b * p.H + y) * p.W + x0;
  if (x0 + 4 <= p.W && ((uintptr_t)o & 3) == 0) {
    *(uint32_t*)o = packed;
  } else {
    for (int k = 0; k < 4; ++k)
      if (x0 + k < p.W) o[k] = (uint8_t)(packed >> (8 * k));
  }
}

// ---------------------------------------------------------------------------------------------- hysteresis
struct HystP {
  int H, W;
  long npix;                                      // B H W
  const uint8_t* state;
  int* label;                                     // [B H W]: the parent's pixel index over the whole batch, -1 where the state is 0
  uint8_t* flag;                                  // [B H W]: 1 at the root of a component that holds a strong pixel
  void* out;
};

OMG_DEV int ld_label(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x: a parent is never above its child, so the walk ends
OMG_DEV int find_root(const int* label, int x) {
  for (;;) {
    const int q = ld_label(label + x);
    if (q == x) return x;
    x = q;
  }
}

// (a) labels of a tile to their fixpoint in LDS: min over the 8 neighbours, then pointer jumping, until a sweep changes nothing
__global__ __launch_bounds__(256) void canny_label_tile_kernel(HystP p) {
  __shared__ int lab[CN_MH * CN_MW];
  const int tx0 = blockIdx.x * CN_TW, ty0 = blockIdx.y * CN_TH;
  const long b = blockIdx.z;
  for (int q = threadIdx.x; q < CN_MH * CN_MW; q += 256) lab[q] = CN_NONE;
  __syncthreads();
  int own[4];                                     // the lane's pixels in the padded tile, -1: outside the image or no candidate
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = threadIdx.x + 256 * k;
    const int ly = t >> 6, lx = t & 63;
    const int y = ty0 + ly, x = tx0 + lx;
    own[k] = -1;
    if (y < p.H && x < p.W) {
      const long g = (b * p.H + y) * p.W + x;
      p.flag[g] = 0;
      if (p.state[g] != 0) {
        own[k] = (ly + 1) * CN_MW + lx + 1;
        lab[own[k]] = own[k];
      } else {
        p.label[g] = -1;
      }
    }
  }
  __syncthreads();
  for (;;) {
    int changed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = own[k];
      if (q < 0) continue;
      const int l = lab[q];
      int m = l;
      m = min(m, min(min(lab[q - CN_MW - 1], lab[q - CN_MW]), lab[q - CN_MW + 1]));
      m = min(m, min(lab[q - 1], lab[q + 1]));
      m = min(m, min(min(lab[q + CN_MW - 1], lab[q + CN_MW]), lab[q + CN_MW + 1]));
      if (m < l) { lab[q] = m; changed = 1; }     // a neighbour's label read while it falls is still one of this component
    }
    if (!__syncthreads_or(changed)) break;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = own[k];
      if (q < 0) continue;
      int l = lab[q];
      for (;;) {                                  // labels only fall and lab[l] <= l: the walk ends at a pixel that labels itself
        const int l2 = lab[l];
        if (l2 >= l) break;
        l = l2;
      }
      lab[q] = l;
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int q = own[k];
    if (q < 0) continue;
    const int t = threadIdx.x + 256 * k;
    const int r = lab[q];
    const int ry = r / CN_MW - 1, rx = r - (ry + 1) * CN_MW - 1;
    p.label[(b * p.H + ty0 + (t >> 6)) * p.W + tx0 + (t & 63)] = (int)((b * p.H + ty0 + ry) * p.W + tx0 + rx);
  }
}

OMG_DEV void unite(int* label, int a, int b) {
  for (;;) {
    a = find_root(label, a);
    b = find_root(label, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }                // a > b: a's tree goes under b
    const int old = atomicMin(label + a, b);
    if (old == a) return;                                        // a was still a root
    a = old;                                                     // somebody moved a first: go on from where it went
  }
}

// (b) one lane per pixel of a tile's last column (the three neighbours to the right) or last row (the three below), where a next tile exists
__global__ __launch_bounds__(256) void canny_border_union_kernel(HystP p, int nv, int nh, long per_image, long total) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long b = t / per_image;
  long r = t - b * per_image;
  int x, y, dx0, dx1, dy0, dy1;
  if (r < (long)nv * p.H) {
    x = (int)(r / p.H) * CN_TW + CN_TW - 1; y = (int)(r % p.H);
    dx0 = dx1 = 1; dy0 = -1; dy1 = 1;
  } else {
    r -= (long)nv * p.H;
    y = (int)(r / p.W) * CN_TH + CN_TH - 1; x = (int)(r % p.W);
    dy0 = dy1 = 1; dx0 = -1; dx1 = 1;
  }
  const long base = b * p.H * p.W;
  const long g = base + (long)y * p.W + x;
  if (p.state[g] == 0) return;
  for (int dy = dy0; dy <= dy1; ++dy)
    for (int dx = dx0; dx <= dx1; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if (yy < 0 || yy >= p.H || xx < 0 || xx >= p.W) continue;
      const long n = base + (long)yy * p.W + xx;
      if (p.state[n] != 0) unite(p.label, (int)g, (int)n);
    }
}

// (c) every label to its root (no union runs beside this kernel: any parent read is an ancestor); strong pixels mark their root
__global__ __launch_bounds__(256) void canny_flatten_kernel(HystP p) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= p.npix) return;
  const int st = p.state[g];
  if (st == 0) return;
  const int r = find_root(p.label, (int)g);
  p.label[g] = r;
  if (st >= 2) p.flag[r] = 1;                                    // every writer stores the same byte
}

// (d) FORM 0: uint8 [B, H, W]; 1: uint8 [B, H, W, 3]; 2: planar [B, 3, H, W] of E holding 0 and 1
template <int FORM, typename E>
__global__ __launch_bounds__(256) void canny_edges_kernel(HystP p, E one) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= p.npix) return;
  const bool on = p.state[g] != 0 && p.flag[p.label[g]] != 0;
  if constexpr (FORM == 0) {
    ((uint8_t*)p.out)[g] = on ? 255 : 0;
  } else if constexpr (FORM == 1) {
    uint8_t* o = (uint8_t*)p.out + 3 * g;
    const uint8_t v = on ? 255 : 0;
    o[0] = v; o[1] = v; o[2] = v;
  } else {
    const long plane = (long)p.H * p.W;
    const long b = g / plane;
    E* o = (E*)p.out + 2 * b * plane + g;                        // b 3 plane + (g - b plane)
    const E v = on ? one : (E)0;
    o[0] = v; o[plane] = v; o[2 * plane] = v;
  }
}

bool canny_sizes_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && W >= 1 && B <= 65535 && (H + CN_TH - 1) / CN_TH <= 65535 && (long)B * H * W < (1L << 31) / 4;
}

}  // namespace

extern "C" int omg_canny_nms(int B, int H, int W, int C, const uint8_t* image, int low, int high, uint8_t* state, void* stream) {
  OMG_REQUIRE(image && state, "omg_canny_nms: null operand");
  OMG_REQUIRE(C == 1 || C == 3, "omg_canny_nms: C is 1 or 3");
  OMG_REQUIRE(canny_sizes_ok(B, H, W), "omg_canny_nms: B, H, W >= 1, B <= 65535, H <= 16 * 65535, B H W < 2^29");
  OMG_REQUIRE(low >= 0 && high >= low, "omg_canny_nms: 0 <= low <= high");
  NmsP p{};
  p.H = H; p.W = W; p.low = low; p.high = high; p.total = (long)B * H * W * C; p.in = image; p.state = state;
  dim3 grid((W + CN_TW - 1) / CN_TW, (H + CN_TH - 1) / CN_TH, B);
  if (C == 1) OMG_LAUNCH(canny_nms_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else OMG_LAUNCH(canny_nms_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, p);
  return omg_check_launch("canny_nms");
}

// labels (int32) in front, flags (bytes) behind them
extern "C" int64_t omg_canny_hysteresis_ws_bytes(int B, int H, int W) {
  if (!canny_sizes_ok(B, H, W)) return 0;
  const int64_t n = (int64_t)B * H * W;
  return (n * 5 + 15) / 16 * 16;
}

extern "C" int omg_canny_hysteresis(int B, int H, int W, const uint8_t* state, void* workspace, int out_form, int out_dtype, void* out,
                                    void* stream) {
  OMG_REQUIRE(state && workspace && out, "omg_canny_hysteresis: null operand");
  OMG_REQUIRE(canny_sizes_ok(B, H, W), "omg_canny_hysteresis: B, H, W >= 1, B <= 65535, H <= 16 * 65535, B H W < 2^29");
  OMG_REQUIRE((uintptr_t)workspace % 4 == 0, "omg_canny_hysteresis: 4-byte aligned workspace");
  OMG_REQUIRE(out_form >= 0 && out_form <= 2, "omg_canny_hysteresis: out_form 0 (uint8 HW), 1 (uint8 HW3) or 2 (planar 3HW)");
  if (out_form == 2) {
    OMG_REQUIRE(out_dtype == OMG_F16 || out_dtype == OMG_BF16 || out_dtype == OMG_F32, "omg_canny_hysteresis: out_dtype of the planar output");
    OMG_REQUIRE((uintptr_t)out % 4 == 0, "omg_canny_hysteresis: 4-byte aligned planar output");
  }
  hipStream_t s = (hipStream_t)stream;
  HystP p{};
  p.H = H; p.W = W; p.npix = (long)B * H * W; p.state = state; p.label = (int*)workspace; p.flag = (uint8_t*)workspace + 4 * p.npix;
  p.out = out;
  const int gx = (W + CN_TW - 1) / CN_TW, gy = (H + CN_TH - 1) / CN_TH;
  OMG_LAUNCH(canny_label_tile_kernel, dim3(gx, gy, B), dim3(256), 0, s, p);
  int rc = omg_check_launch("canny_label_tile");
  if (rc) return rc;
  const int nv = gx - 1, nh = gy - 1;                            // tile borders with a tile behind them
  const long per_image = (long)nv * H + (long)nh * W, total = per_image * B;
  if (total > 0) {                                               // a function of the sizes, not of the data
    OMG_LAUNCH(canny_border_union_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, nv, nh, per_image, total);
    rc = omg_check_launch("canny_border_union");
    if (rc) return rc;
  }
  const dim3 flat((unsigned)((p.npix + 255) / 256));
  OMG_LAUNCH(canny_flatten_kernel, flat, dim3(256), 0, s, p);
  rc = omg_check_launch("canny_flatten");
  if (rc) return rc;
  if (out_form == 0) OMG_LAUNCH((canny_edges_kernel<0, uint8_t>), flat, dim3(256), 0, s, p, (uint8_t)255);
  else if (out_form == 1) OMG_LAUNCH((canny_edges_kernel<1, uint8_t>), flat, dim3(256), 0, s, p, (uint8_t)255);
  else if (out_dtype == OMG_F32) OMG_LAUNCH((canny_edges_kernel<2, uint32_t>), flat, dim3(256), 0, s, p, 0x3f800000u);
  else OMG_LAUNCH((canny_edges_kernel<2, uint16_t>), flat, dim3(256), 0, s, p, (uint16_t)(out_dtype == OMG_F16 ? 0x3c00 : 0x3f80));
  return omg_check_launch("canny_edges");
}
