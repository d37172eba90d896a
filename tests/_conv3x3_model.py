"""CPU references for the dense 3x3 NHWC convolution, the depthwise 3x3 convolution and the bicubic upsample-add of csrc/effvit.hip
(omg_conv3x3_nhwc_act / omg_conv3x3_nhwc_ex, omg_dwconv3x3_act, omg_upsample_add_nhwc): plain torch, no GPU.  The case lists of
tests/test_conv3x3_edges_gpu.py live here too, so that tests/test_conv3x3_model.py can show without a GPU that the checks reject a
subtly wrong kernel at the very shapes the GPU suite runs.

Layouts: x [B, H, W, Cin], w [Cout, 3, 3, Cin], bias [Cout], residual and result [B, Hout, Wout, Cout] (the references return
[B Hout Wout, Cout] rows); depthwise x [B H W, C] rows, taps [9, C]; Hout = (H - 1) // stride + 1.

  *_truth   float64 on the STORED 16-bit operands (F.conv2d with explicit padding, tests/dpt_torch.same_pad for `same` at stride 2,
            F.interpolate(mode="bicubic", align_corners=False)): the reference of record.  Returned with the activation allowance.
  *_ref32   the same computation evaluated by torch in fp32, returned as float64: the case's conditioning.
  held      the rule of tests/_litemla_model.py, elementwise, no element excluded:

                |out - truth|  <=  ulp16(truth) / 2  +  C_RULE * E32  [+ activation allowance]

            E32 = max |ref32 - truth| over the case, floored at 2^-23 max |truth|; C_RULE = 4.

The activation allowance (derived, not measured).  The kernels' tanh GELU is  gelu_tanh_f(x) = x * rcp(1 + __expf(-z)),
z = 1.5957691 u,  u = x (1 + 0.044715 x^2):  x sigmoid(z), the same function as 0.5 x (1 + tanh(z / 2)).  What is stored is x s
with s = 1 / (1 + e), e = exp(-z), so an absolute error ds of the sigmoid costs |x| ds.  A relative error r of e moves s by
s (1 - s) r.  Step by step, in units of 2^-24 (one fp32 rounding, relative):
  * the argument: z comes out of about six roundings (the polynomial, the constant, __expf's own scaling by log2 e), a relative
    error of 6 2^-24, which is a relative error |z| 6 2^-24 of e.  z s (1 - s) <= 0.224 for every z (checked in
    tests/test_conv3x3_model.py), so ds stays below about 1.4 2^-24;
  * v_exp_f32 at 1 ulp, as the ISA manual states it: r = 2 2^-24, through s (1 - s) <= 1/4 a ds of at most 0.5 2^-24;
  * the add 1 + e rounds once: a relative 2^-24 of s, and s <= 1;
  * v_rcp_f32 at 1 ulp: 2 2^-24 of s;
  * the final multiply x s rounds once: 2^-24.
  Total below (1.4 + 0.5 + 1 + 2 + 1) 2^-24 |x| < 6 2^-24 |x| < 2^-21 |x|.  ALLOW = 2^-20 |p| per activated element is granted, p
  being the float64 pre-activation (or the input, for gelu_in): a factor of 2 over the derivation, for instruction accuracies that
  nobody here has verified.  For gelu_in the allowance of every input tap reaches the output through its weight,
  sum |w| 2^-20 |x|, and a GELU of the output multiplies what arrives by at most sup |gelu'| (GELU_SLOPE, evaluated below, 1.13)
  before its own 2^-20 |p| is added.  ReLU, bias and residual are exact or single fp32 roundings inside the E32 floor.

Emulations, for tests/test_conv3x3_model.py and the bitwise depthwise comparison:
  dwconv3x3_emulation  dwconv3x3_kernel without GELU, bit for bit: fp32, starts from the bias (or 0), fma(x, w, acc) per tap, ty outer
                       and tx inner, out-of-image taps skipped, one rounding at the store (`.to(dtype)` of what is returned).  It is
                       the argument of dwconv_emulation in tests/_litemla_model.py extended by the stride: a product of two 16-bit
                       values is exact in fp32, and the fma is taken in float64 and rounded to fp32.
  conv3x3_emulation    the dense kernel's algorithm in fp32: K = (tap, cin padded to 8) tap-major, accumulated 32 at a time.  The
                       MFMA's internal order is not specified, so this is NOT bit-exact and serves the fault tests only.
  upsample_emulation   upsample_add_kernel's algorithm in fp32: four taps along x, then along y, clamped indices.
Each takes one fault at a time (DENSE_FAULTS, DW3_FAULTS, UP_FAULTS; described at the functions)."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests._litemla_model import BF16, C_RULE, F16, dwconv_inputs, held, name, ulp16  # noqa: F401  (re-exported)
from tests.dpt_torch import same_pad

ALLOW = 2.0 ** -20


def gelu(x):
    return F.gelu(x, approximate="tanh")


def _gelu_slope():
    p = torch.linspace(-8, 8, 160001, dtype=torch.float64, requires_grad=True)
    gelu(p).sum().backward()
    return float(p.grad.abs().max())


GELU_SLOPE = _gelu_slope()      # sup |gelu'| = 1.129 (at p = 1.48); beyond |p| = 8 the slope is 0 or 1 to 1e-13


def gelu_f32(x):
    """gelu_tanh_f in fp32 torch operations (not bit-exact: exp and the reciprocal are the host's)."""
    u = x * (0.044715 * x * x + 1.0)
    return x * (1.0 / (1.0 + torch.exp(-1.5957691216057308 * u)))


def out_size(n, stride):
    return (n - 1) // stride + 1


# ------------------------------------------------------------------------------------------------------------------ the dense kernel
def _dense(x, w, bias, res, stride, act, relu_in, same, ft):
    Cout = w.shape[0]
    xi = x.to(ft).permute(0, 3, 1, 2)
    if relu_in:
        xi = torch.relu(xi)
    wi = w.to(ft).permute(0, 3, 1, 2)
    b = None if bias is None else bias.to(ft)
    if same and stride == 2:
        pre = F.conv2d(same_pad(xi, 3, 2), wi, b, stride=2)
    else:
        pre = F.conv2d(xi, wi, b, stride=stride, padding=1)
    assert pre.shape[2:] == (out_size(x.shape[1], stride), out_size(x.shape[2], stride))
    pre = pre.permute(0, 2, 3, 1).reshape(-1, Cout)
    y = gelu(pre) if act == 1 else torch.relu(pre) if act == 2 else pre
    if res is not None:
        y = y + res.to(ft).reshape(-1, Cout)
    return y, pre


def dense_truth(x, w, bias=None, res=None, stride=1, act=0, relu_in=False, same=False):
    """-> (truth [M, Cout] float64, allowance [M, Cout] float64 or None)."""
    y, pre = _dense(x, w, bias, res, stride, act, relu_in, same, torch.float64)
    return y, (ALLOW * pre.abs() if act == 1 else None)


def dense_ref32(x, w, bias=None, res=None, stride=1, act=0, relu_in=False, same=False):
    return _dense(x, w, bias, res, stride, act, relu_in, same, torch.float32)[0].double()


DENSE_FAULTS = ("col_tile_offset", "drop_last_chunk", "wrap_row", "wrap_batch", "same_origin", "stride_phase", "residual_before_act",
                "relu_on_residual", "cin_pad_garbage")


def conv3x3_emulation(x, w, bias=None, res=None, stride=1, act=0, relu_in=False, same=False, fault=None):
    """conv3x3_kernel in fp32, unrounded, as float64 [M, Cout].  Faults:
    col_tile_offset      output channels >= 128 take the weights of channel c - 128 (n0 forgotten in the weight load).
    drop_last_chunk      the last group of fewer than 4 K vectors (KV % 4 of them) is never multiplied.
    wrap_row             a tap that leaves the image on the left reads the linear address: the previous row's last pixel.
    wrap_batch           a tap that leaves the image vertically reads the neighbouring image of the batch.
    same_origin          padding 1 in front of an even size under `same` (the origin of padding=1).
    stride_phase         stride 2 samples the odd pixels.
    residual_before_act  act(pre + residual).
    relu_on_residual     with relu_in, the residual is read through the ReLU too.
    cin_pad_garbage      for Cin < 8 the lanes c >= Cin read on instead of zero: the next pixel's channels in X and the next tap's in W
                         (in one operand alone the other's zeros would hide it from every finite input)."""
    assert fault is None or fault in DENSE_FAULTS, fault
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    M, CinP = B * Ho * Wo, (Cin + 7) & ~7
    tf = same and stride == 2
    pad_t, pad_l = (H & 1 if tf else 1), (W & 1 if tf else 1)
    if fault == "same_origin":
        pad_t = pad_l = 1
    phase = 1 if fault == "stride_phase" and stride == 2 else 0
    garbage = fault == "cin_pad_garbage" and Cin < 8
    xf = x.float()
    if relu_in:
        xf = torch.relu(xf)
    xflat, wflat = xf.reshape(-1), w.float().reshape(-1)
    b = torch.arange(B)[:, None, None]
    oy, ox = torch.arange(Ho)[None, :, None], torch.arange(Wo)[None, None, :]
    c = torch.arange(CinP)[None, :]
    lane = c < Cin

    def read(flat, idx, ok):
        ok = ok & (idx < flat.numel()) if garbage else ok & lane
        return torch.where(ok, flat[idx.clamp(0, flat.numel() - 1)], torch.zeros(()))

    A, Wm = torch.zeros(M, 9 * CinP), torch.zeros(Cout, 9 * CinP)
    for tap in range(9):
        ty, tx = divmod(tap, 3)
        iy, ix = oy * stride - pad_t + ty + phase, ox * stride - pad_l + tx + phase
        pix = (b * H + iy) * W + ix
        oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
        if fault == "wrap_row":
            okx = okx | ((ix < 0) & (pix >= 0))
        if fault == "wrap_batch":
            oky = (b * H + iy >= 0) & (b * H + iy < B * H)
        ok = (oky & okx).expand(B, Ho, Wo).reshape(M, 1)
        A[:, tap * CinP:(tap + 1) * CinP] = read(xflat, pix.expand(B, Ho, Wo).reshape(M, 1) * Cin + c, ok)
        wo = (torch.arange(Cout)[:, None] * 9 + tap) * Cin
        Wm[:, tap * CinP:(tap + 1) * CinP] = read(wflat, wo + c, torch.ones(Cout, 1, dtype=torch.bool))
    if fault == "col_tile_offset" and Cout > 128:
        Wm = torch.cat([Wm[:128], Wm[:Cout - 128]])
    KV = 9 * CinP // 8
    nchunks = (KV + 3) // 4
    acc = torch.zeros(M, Cout)
    for kc in range(nchunks):
        if fault == "drop_last_chunk" and kc == nchunks - 1 and KV % 4:
            continue
        k0, k1 = 32 * kc, min(32 * kc + 32, 9 * CinP)
        acc = acc + A[:, k0:k1] @ Wm[:, k0:k1].t()
    if bias is not None:
        acc = acc + bias.float()
    r = None if res is None else res.float().reshape(M, Cout)
    if r is not None and fault == "relu_on_residual" and relu_in:
        r = torch.relu(r)
    if r is not None and fault == "residual_before_act":
        acc, r = acc + r, None
    acc = gelu_f32(acc) if act == 1 else torch.relu(acc) if act == 2 else acc
    if r is not None:
        acc = acc + r
    return acc.double()


Dense = namedtuple("Dense", "cin cout B H W stride same bias act res relu_in entry family")

PAIRS = [(1, 8), (2, 40), (5, 200), (7, 136), (8, 72), (8, 264), (24, 128), (40, 136), (40, 256), (256, 264), (768, 256)]
# (B, H, W): one pixel, one row, one column, 2 x 2 (1 x 1 at stride 2), odd x odd, even x even, three images whose boundaries fall
# inside a wave, and M = 127 / 128 / 129 at stride 1
PIXELS = [(1, 1, 1), (1, 1, 6), (1, 6, 1), (1, 2, 2), (1, 7, 9), (1, 8, 6), (3, 7, 9), (1, 127, 1), (2, 8, 8), (3, 1, 43)]
BIG_PIXELS = {(256, 264): [(3, 7, 9), (1, 8, 6), (1, 1, 6), (2, 8, 8)], (768, 256): [(2, 9, 7), (1, 2, 2), (1, 1, 1)]}
MODES = [(1, False), (2, False), (2, True), (1, True)]            # `same` at stride 1 is padding 1: the flag must change nothing
# (bias, act, residual, relu_in, through the _ex entry)
EPILOGUES = [(True, 0, False, False, False), (False, 1, True, False, False), (True, 2, True, False, True), (True, 0, True, True, True),
             (False, 1, False, False, True), (True, 1, True, True, True)]
OFFSET_PAIRS = [(5, 200), (40, 136), (256, 264), (768, 256)]


def dense_cases(pair, family="plain"):
    """The cases of one (Cin, Cout): every pixel shape x every mode, the epilogues taken in turn."""
    cin, cout = pair
    i, cases = PAIRS.index(pair), []
    for B, H, W in BIG_PIXELS.get(pair, PIXELS):
        for stride, same in MODES:
            bias, act, res, relu_in, ex = EPILOGUES[(i + len(cases)) % len(EPILOGUES)]
            cases.append(Dense(cin, cout, B, H, W, stride, same, bias, act, res, relu_in, "ex" if ex or same else "act", family))
    return cases


def dense_tag(c):
    return (f"dense {c.family} {c.cin}->{c.cout} {c.B}x{c.H}x{c.W} s{c.stride} same{int(c.same)} bias{int(c.bias)} act{c.act} res{int(c.res)} "
            f"relu_in{int(c.relu_in)} {c.entry}")


def dense_inputs(c, dtype, seed):
    """plain: x = randn, w = randn / sqrt(9 Cin), bias = randn / 2, residual = randn (the scales of tests/test_effvit_gpu.py).
    offset: x = 100 + randn / 4 and the weights of every output channel shifted to zero mean, so that the sum cancels."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(c.B, c.H, c.W, c.cin, generator=g)
    w = torch.randn(c.cout, 3, 3, c.cin, generator=g) * (1.0 / (9 * c.cin)) ** 0.5
    if c.family == "offset":
        x = 100.0 + x / 4
        w = w - w.mean(dim=(1, 2, 3), keepdim=True)
    else:
        assert c.family == "plain", c.family
    bias = (torch.randn(c.cout, generator=g) * 0.5).to(dtype) if c.bias else None
    res = torch.randn(c.B, out_size(c.H, c.stride), out_size(c.W, c.stride), c.cout, generator=g).to(dtype) if c.res else None
    return x.to(dtype), w.to(dtype), bias, res


def dense_kwargs(c):
    return dict(stride=c.stride, act=c.act, relu_in=c.relu_in, same=c.same)


EXACT_PIXELS = [(3, 7, 9), (2, 8, 6)]             # odd and even extents: both origins of `same`
EXACT_BIG_PIXELS = [(2, 9, 7), (1, 8, 6)]
EXACT_MODES = [(1, False), (2, False), (2, True)]


def exact_pixels(pair):
    return EXACT_BIG_PIXELS if pair in BIG_PIXELS else EXACT_PIXELS


def dense_integers(cin, cout, B, H, W, stride, seed=5):
    """The generator of test_conv3x3_exact_on_small_integers in NHWC: x in {-1, 0, 1}, w in {-1, 0, 1} at density 0.25, bias and
    residual in -4..4; fp32 tensors of integers."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (B, H, W, cin), generator=g).float()
    w = torch.randint(-1, 2, (cout, 3, 3, cin), generator=g).float() * (torch.rand(cout, 3, 3, cin, generator=g) < 0.25)
    b = torch.randint(-4, 5, (cout,), generator=g).float()
    r = torch.randint(-4, 5, (B, out_size(H, stride), out_size(W, stride), cout), generator=g).float()
    return x, w, b, r


# -------------------------------------------------------------------------------------------------------------- the depthwise kernel
def _dw(x, taps, bias, B, H, W, stride, gelu_out, gelu_in, ft):
    C = x.shape[1]
    xi = x.to(ft).reshape(B, H, W, C).permute(0, 3, 1, 2)
    if gelu_in:
        xi = gelu(xi)
    wi = taps.to(ft).t().reshape(C, 1, 3, 3)
    pre = F.conv2d(xi, wi, None if bias is None else bias.to(ft), stride=stride, padding=1, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
    return (gelu(pre) if gelu_out else pre), pre


def dw_truth(x, taps, bias, B, H, W, stride, gelu_out=False, gelu_in=False):
    """-> (truth [Mout, C] float64, allowance or None)."""
    y, pre = _dw(x, taps, bias, B, H, W, stride, gelu_out, gelu_in, torch.float64)
    allow = None
    if gelu_in:
        C = x.shape[1]
        xa = x.double().abs().reshape(B, H, W, C).permute(0, 3, 1, 2)
        wa = taps.double().abs().t().reshape(C, 1, 3, 3)
        allow = ALLOW * F.conv2d(xa, wa, None, stride=stride, padding=1, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
    if gelu_out:
        allow = ALLOW * pre.abs() if allow is None else GELU_SLOPE * allow + ALLOW * pre.abs()
    return y, allow


def dw_ref32(x, taps, bias, B, H, W, stride, gelu_out=False, gelu_in=False):
    return _dw(x, taps, bias, B, H, W, stride, gelu_out, gelu_in, torch.float32)[0].double()


DW3_FAULTS = ("swap_ty_tx", "wrap_batch", "bias_after_round", "gelu_in_on_padding_as_nonzero")


def dwconv3x3_emulation(x, taps, bias, B, H, W, stride, fault=None, gelu_out=False, gelu_in=False):
    """dwconv3x3_kernel in fp32, unrounded: -> fp32 [B Hout Wout, C]; `.to(x.dtype)` is what the kernel stores, bit for bit while
    gelu_out and gelu_in are off (with them the host's exp stands in for the GPU's: for the rule only).  Faults:
    swap_ty_tx                      tap (ty, tx) takes the weight of (tx, ty).
    wrap_batch                      a tap that leaves the image vertically reads the neighbouring image of the batch.
    bias_after_round                the bias is added to the rounded sum, which is rounded again (returned rounded, as fp32).
    gelu_in_on_padding_as_nonzero   under gelu_in an out-of-image tap is not skipped: it enters as the gate sigmoid(0) = 0.5 of the
                                    activation instead of gelu(0) = 0."""
    assert fault is None or fault in DW3_FAULTS, fault
    C = x.shape[1]
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xf = x.float().reshape(B * H * W, C)
    if gelu_in:
        xf = gelu_f32(xf)
    late = fault == "bias_after_round"
    acc = (bias.float() if bias is not None and not late else torch.zeros(C)).expand(B * Ho * Wo, C).clone()
    b = torch.arange(B)[:, None, None]
    oy, ox = torch.arange(Ho)[None, :, None], torch.arange(Wo)[None, None, :]
    for ty in range(3):
        for tx in range(3):
            iy, ix = oy * stride - 1 + ty, ox * stride - 1 + tx
            oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
            if fault == "wrap_batch":
                oky = (b * H + iy >= 0) & (b * H + iy < B * H)
            ok = (oky & okx).expand(B, Ho, Wo).reshape(-1, 1)
            pix = ((b * H + iy) * W + ix).expand(B, Ho, Wo).reshape(-1).clamp(0, B * H * W - 1)
            wt = taps[tx * 3 + ty if fault == "swap_ty_tx" else ty * 3 + tx].double()
            xv = xf[pix].double()
            if fault == "gelu_in_on_padding_as_nonzero" and gelu_in:
                xv, ok = torch.where(ok, xv, torch.full((), 0.5, dtype=torch.float64)), torch.ones_like(ok)
            acc = torch.where(ok, (acc.double() + xv * wt).float(), acc)
    if late:
        acc = acc.to(x.dtype).float() + (bias.float() if bias is not None else 0.0)
        return acc.to(x.dtype).float()
    return gelu_f32(acc) if gelu_out else acc


DW_CHANNELS = [8, 24, 264]
DW_PIXELS = [(3, 1, 1), (3, 1, 6), (3, 6, 1), (3, 2, 2), (3, 7, 9), (3, 8, 6)]


# ------------------------------------------------------------------------------------------------------------------ bicubic upsample
def _up(x, Ho, Wo, y0, accumulate, ft):
    C = x.shape[3]
    up = F.interpolate(x.to(ft).permute(0, 3, 1, 2), size=(Ho, Wo), mode="bicubic", align_corners=False).permute(0, 2, 3, 1)
    if accumulate:
        up = up + y0.to(ft)
    return up.reshape(-1, C)


def up_truth(x, Ho, Wo, y0=None, accumulate=False):
    return _up(x, Ho, Wo, y0, accumulate, torch.float64)


def up_ref32(x, Ho, Wo, y0=None, accumulate=False):
    return _up(x, Ho, Wo, y0, accumulate, torch.float32).double()


UP_FAULTS = ("a_minus_half", "align_corners", "zero_pad_instead_of_clamp", "swapped_scales")


def _cubic_w(t, A):
    x0, x3, x2 = t + 1.0, 2.0 - t, 1.0 - t
    return torch.stack([((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A, ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0,
                        ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0, ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A], dim=1)


def upsample_emulation(x, Ho, Wo, y0=None, accumulate=False, fault=None):
    """upsample_add_kernel in fp32, unrounded, as float64 [B Ho Wo, C].  Faults: a_minus_half (the cubic's A = -0.5, Keys' kernel, for
    torch's -0.75); align_corners (source coordinate dst (in - 1) / (out - 1)); zero_pad_instead_of_clamp (a tap outside the image
    contributes 0); swapped_scales (in / out of the rows used along x and that of the columns along y)."""
    assert fault is None or fault in UP_FAULTS, fault
    B, Hi, Wi, C = x.shape
    f32 = torch.float32
    sy, sx = torch.tensor(Hi, dtype=f32) / torch.tensor(Ho, dtype=f32), torch.tensor(Wi, dtype=f32) / torch.tensor(Wo, dtype=f32)
    if fault == "swapped_scales":
        sy, sx = sx, sy
    A = -0.5 if fault == "a_minus_half" else -0.75

    def axis(n_in, n_out, s):
        o = torch.arange(n_out, dtype=f32)
        r = o * (float(n_in - 1) / float(max(n_out - 1, 1))) if fault == "align_corners" else s * (o + 0.5) - 0.5
        fl = torch.floor(r)
        wt = _cubic_w(r - fl, A)
        idx = fl.long()[:, None] - 1 + torch.arange(4)[None, :]
        if fault == "zero_pad_instead_of_clamp":
            wt = torch.where((idx >= 0) & (idx < n_in), wt, torch.zeros(()))
        return idx.clamp(0, n_in - 1), wt

    iy, wy = axis(Hi, Ho, sy)
    ix, wx = axis(Wi, Wo, sx)
    xf = x.float()
    out = torch.zeros(B, Ho, Wo, C)
    for i in range(4):
        rows = xf[:, iy[:, i]]                                               # [B, Ho, Wi, C]
        row = torch.zeros(B, Ho, Wo, C)
        for j in range(4):
            row = row + rows[:, :, ix[:, j]] * wx[None, None, :, j, None]
        out = out + row * wy[None, :, i, None, None]
    if accumulate:
        out = out + y0.float()
    return out.reshape(-1, C).double()


# (Hin, Win) -> (Hout, Wout): non-integer and non-square both ways, identity, every tap clamped, a downscale, the neck's 8x
RESIZES = [((5, 7), (8, 9)), ((7, 5), (9, 8)), ((6, 6), (6, 6)), ((1, 4), (3, 8)), ((4, 1), (8, 3)), ((16, 12), (6, 5)), ((8, 8), (64, 64))]
UP_CHANNELS = [8, 264]


def up_inputs(B, hin, win, hout, wout, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, hin, win, C, generator=g).to(dtype), torch.randn(B, hout, wout, C, generator=g).to(dtype)
