"""The kernels of the DPT depth estimator (-m gpu): every new entry of omg_amd/csrc/dpt.hip and omg_conv3x3_nhwc_ex against torch
fp32 / float64 on the same 16-bit operands, at the smallest shapes that can go wrong; outputs canary-filled; fp16 and bf16.

Bounds.  The kernels accumulate in fp32 and round once, so against the fp32 reference the error is half an ulp of the storage dtype at
the value plus the fp32 summation-order noise (K <= 9 * 24 terms: far below that ulp).  The bound is ONE ulp of the storage dtype at
the reference's largest magnitude.  The max-pool selects stored values: it is compared with ``torch.equal``.  The fp32 row dot is held
to 2^-20 of sum |x w| (K = 32 fp32 roundings).  The tail's bytes are compared with a float64 restatement: equal, except where the
float64 value x 255 lies within 1e-3 of an integer, where +-1 is allowed, for at most 1 % of the pixels."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from omg_amd import ops
from tests.dpt_torch import same_pad

DTYPES = [torch.float16, torch.bfloat16]
SIZES = [(8, 6), (7, 9), (1, 1)]
CANARY = 1232.0          # a value of the fp16 and of the bf16 grid
RECORDING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3x3_nhwc_act_recording.npz")


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float16):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def ulp(dtype, mag):
    bits = 10 if dtype == torch.float16 else 7
    return 2.0 ** (math.floor(math.log2(max(mag, 2.0 ** -14))) - bits)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def canary_out(shape, dtype, dev, extra=64, value=CANARY):
    n = math.prod(shape)
    flat = torch.full((n + extra,), value, dtype=dtype, device=dev)
    return flat, flat[:n].view(shape)


def close(tag, dtype, got_nchw, ref32):
    err = (got_nchw.float().cpu() - ref32).abs().max().item()
    bound = ulp(dtype, ref32.abs().max().item())
    print(f"{tag}: max |d| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (tag, err, bound)


def canary_ok(flat, n):
    assert bool((flat[n:].float() == CANARY).all()), "wrote past the output"


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES + [(33, 18)])
@pytest.mark.parametrize("in32", [False, True])
def test_stem_conv(dev, dtype, size, in32):
    H, W = size
    B, cout = 2, 32
    x = rnd(B, 3, H, W, seed=1, dtype=dtype)
    w = rnd(cout, 3, 7, 7, seed=2, scale=0.1, dtype=dtype)
    ref = F.conv2d(same_pad(x.float(), 7, 2), w.float(), stride=2)
    shape = (B, (H + 1) // 2, (W + 1) // 2, cout)
    assert tuple(ref.shape) == (B, cout) + shape[1:3]
    flat, out = canary_out(shape, dtype, dev)
    xin = (x.float() if in32 else x).to(dev)
    ops.dpt_stem_conv(xin, ops.pack_dpt_stem_weight(w).to(dev), out=out)
    canary_ok(flat, out.numel())
    close(f"stem {size} {dtype} in32={in32}", dtype, nchw(out), ref)


# ------------------------------------------------------------------------------------------------ 3x3 convolution
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("cin,cout", [(8, 40), (24, 8)])
def test_conv3x3_same_stride2(dev, dtype, size, cin, cout):
    H, W = size
    B = 2
    x, w, b = rnd(B, cin, H, W, seed=3, dtype=dtype), rnd(cout, cin, 3, 3, seed=4, scale=0.2, dtype=dtype), rnd(cout, seed=5, dtype=dtype)
    ref = F.relu(F.conv2d(same_pad(x.float(), 3, 2), w.float(), b.float(), stride=2))
    shape = (B, (H + 1) // 2, (W + 1) // 2, cout)
    flat, out = canary_out(shape, dtype, dev)
    ops.conv3x3_nhwc_ex(nhwc(x).to(dev), nhwc(w).to(dev), stride=2, bias=b.to(dev), act=2, same=True, out=out)
    canary_ok(flat, out.numel())
    close(f"conv3x3 SAME/2 {size} {cin}->{cout} {dtype}", dtype, nchw(out), ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [8, 24])
def test_conv3x3_relu_on_load_residual_unactivated(dev, dtype, c):
    """``x + conv(relu(x))``: the convolution sees relu(x), the shortcut x itself (mostly negative, so the two differ everywhere)."""
    B, H, W = 2, 13, 11                                                    # 286 pixels: three blocks of 128
    x = (rnd(B, c, H, W, seed=6, dtype=torch.float32) - 0.8).to(dtype)
    w, b = rnd(c, c, 3, 3, seed=7, scale=0.2, dtype=dtype), rnd(c, seed=8, dtype=dtype)
    ref = F.conv2d(F.relu(x.float()), w.float(), b.float(), padding=1) + x.float()
    flat, out = canary_out((B, H, W, c), dtype, dev)
    xd = nhwc(x).to(dev)
    ops.conv3x3_nhwc_ex(xd, nhwc(w).to(dev), bias=b.to(dev), residual=xd, relu_in=True, out=out)
    canary_ok(flat, out.numel())
    close(f"conv3x3 relu-in + residual C={c} {dtype}", dtype, nchw(out), ref)
    wrong = F.conv2d(F.relu(x.float()), w.float(), b.float(), padding=1) + F.relu(x.float())
    assert (wrong - ref).abs().max().item() > 100 * ulp(dtype, ref.abs().max().item())        # the test can tell the two apart


def test_old_conv_entry_unchanged(dev):
    """omg_conv3x3_nhwc_act with its old arguments against outputs recorded from the library as it was before omg_conv3x3_nhwc_ex and
    the kernel's new arguments existed: bit for bit, at two shapes (stride 1 with GELU and residual; stride 2, Cin = 3)."""
    z = np.load(RECORDING)
    for tag in ("a", "b"):
        dtype = torch.float16 if tag == "a" else torch.bfloat16
        bits = lambda k: torch.from_numpy(z[f"{tag}.{k}"]).view(dtype).to(dev)                # noqa: E731
        x, w, b = bits("x"), bits("w"), bits("bias")
        stride, gelu = int(z[f"{tag}.stride"]), bool(z[f"{tag}.gelu"])
        res = bits("res") if f"{tag}.res" in z.files else None
        got = ops.conv3x3_nhwc_act(x, w, stride=stride, bias=b, gelu=gelu, residual=res)
        assert torch.equal(got.view(torch.int16).cpu(), torch.from_numpy(z[f"{tag}.y"])), tag


# ------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_maxpool_same(dev, dtype, size):
    H, W = size
    B, c = 2, 24
    x = rnd(B, c, H, W, seed=9, dtype=dtype)
    ref = F.max_pool2d(same_pad(x.float(), 3, 2), 3, 2)
    flat, out = canary_out((B, (H + 1) // 2, (W + 1) // 2, c), dtype, dev)
    ops.maxpool3x3s2_nhwc(nhwc(x).to(dev), out=out)
    canary_ok(flat, out.numel())
    assert torch.equal(nchw(out).float().cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_maxpool_all_negative(dev, dtype):
    """An all-negative 8 x 6 input: the padded zero (behind only, at even sizes) wins in the last row and column and nowhere else."""
    B, c, H, W = 1, 8, 8, 6
    x = (-1.0 - rnd(B, c, H, W, seed=10, dtype=torch.float32).abs()).to(dtype)
    got = nchw(ops.maxpool3x3s2_nhwc(nhwc(x).to(dev))).float().cpu()
    assert torch.equal(got, F.max_pool2d(same_pad(x.float(), 3, 2), 3, 2))
    zero = got == 0
    expect = torch.zeros_like(zero)
    expect[:, :, -1, :] = True
    expect[:, :, :, -1] = True
    assert torch.equal(zero, expect)


# ------------------------------------------------------------------------------------------------ GroupNorm + residual + ReLU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,groups", [(16, 8), (8, 8), (64, 8)])
@pytest.mark.parametrize("res,relu", [(False, False), (False, True), (True, True), (True, False)])
def test_groupnorm_res_act(dev, dtype, c, groups, res, relu):
    B, H, W = 2, 7, 9                                                      # HW = 63: no multiple of the pixel rows of a block
    x = rnd(B, H, W, c, seed=11, scale=2.0, dtype=dtype)
    ga, be = (1.0 + 0.2 * rnd(c, seed=12, dtype=torch.float32)).to(dtype), rnd(c, seed=13, scale=0.1, dtype=dtype)
    r = rnd(B, H, W, c, seed=14, dtype=dtype) if res else None
    ref = F.group_norm(nchw(x).double(), groups, ga.double(), be.double(), 1e-5)
    if res:
        ref = ref + nchw(r).double()
    if relu:
        ref = F.relu(ref)
    flat, out = canary_out((B, H, W, c), dtype, dev)
    ops.groupnorm_res_act(x.to(dev), ga.to(dev), be.to(dev), groups, 1e-5, residual=None if r is None else r.to(dev), relu=relu, out=out)
    canary_ok(flat, out.numel())
    close(f"groupnorm C={c} G={groups} res={res} relu={relu} {dtype}", dtype, nchw(out), ref.float())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("std", [0.1, 8.0])
def test_groupnorm_mean_far_from_zero(dev, dtype, std):
    """|mean| >> std: 1e3 +- 1e-1 (a few levels of the fp16 grid, one of bf16's) and 1e3 +- 8; the reference is float64 on the same
    stored values.  Many chunks (96 x 96 x 16) and one."""
    for (H, W) in ((96, 96), (5, 5)):
        B, c, groups = 1, 16, 8
        x = (1000.0 + std * rnd(B, H, W, c, seed=15, dtype=torch.float32)).to(dtype)
        ga, be = torch.ones(c, dtype=dtype), torch.zeros(c, dtype=dtype)
        ref = F.group_norm(nchw(x).double(), groups, ga.double(), be.double(), 1e-5).float()
        got = ops.groupnorm_res_act(x.to(dev), ga.to(dev), be.to(dev), groups, 1e-5)
        close(f"groupnorm 1e3 +- {std} {H}x{W} {dtype}", dtype, nchw(got), ref)


# ------------------------------------------------------------------------------------------------ upsample
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_upsample2x(dev, dtype, size):
    H, W = size
    B, c = 2, 16
    x = rnd(B, c, H, W, seed=16, dtype=dtype)
    ref = F.interpolate(x.float(), scale_factor=2, mode="bilinear", align_corners=True)
    flat, out = canary_out((B, 2 * H, 2 * W, c), dtype, dev)
    ops.upsample2x_bilinear_nhwc(nhwc(x).to(dev), out=out)
    canary_ok(flat, out.numel())
    close(f"upsample {size} {dtype}", dtype, nchw(out), ref)
    if size == (1, 1):
        assert torch.equal(nchw(out).float().cpu(), x.float().expand(B, c, 2, 2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_upsample2x_ramp_exact(dev, dtype):
    """A linear ramp comes back exactly: x[i] = i (2n - 1) sampled at i' (n - 1) / (2n - 1) is the integer i' (n - 1)."""
    n = 6                                                                    # values up to 55: integers of both grids
    i = torch.arange(n, dtype=torch.float32) * (2 * n - 1)
    x = torch.stack([i[:, None].expand(n, n), i[None, :].expand(n, n)], 0)[None].repeat(1, 4, 1, 1).to(dtype)      # along y, along x: 8 channels
    got = nchw(ops.upsample2x_bilinear_nhwc(nhwc(x).to(dev))).float().cpu()
    o = torch.arange(2 * n, dtype=torch.float32) * (n - 1)
    want = torch.stack([o[:, None].expand(2 * n, 2 * n), o[None, :].expand(2 * n, 2 * n)], 0)[None].repeat(1, 4, 1, 1)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ head projection
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowdot(dev, dtype):
    M, c = 300, 32                                                           # two blocks
    x, w, b = rnd(M, c, seed=17, dtype=dtype), rnd(c, seed=18, dtype=dtype), rnd(1, seed=19, dtype=dtype)
    ref = x.double() @ w.double() + b.double()
    flat, out = canary_out((M,), torch.float32, dev)
    ops.rowdot_f32(x.to(dev), w.to(dev), b.to(dev), relu=True, out=out)
    canary_ok(flat, M)
    bound = 2.0 ** -20 * (x.double().abs() @ w.double().abs() + b.double().abs())
    assert bool(((out.cpu().double() - F.relu(ref)).abs() <= bound).all())
    assert bool((out.cpu() == 0).any()) and bool((out.cpu() > 0).any())
    raw = ops.rowdot_f32(x.to(dev), w.to(dev), None, relu=False).cpu().double()
    assert bool(((raw - x.double() @ w.double()).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ get_depth's tail
def cubic64(t):
    A = -0.75
    x0, x2, x3 = t + 1.0, 1.0 - t, 2.0 - t
    return np.stack([((A * x0 - 5 * A) * x0 + 8 * A) * x0 - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
                     ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1, ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A], -1)


def resize64(d, H, W):
    """Bicubic (a = -0.75, align_corners=False, clamped taps) of [h, w] in float64."""
    h, w = d.shape

    def axis(n_in, n_out):
        r = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        f = np.floor(r)
        idx = np.clip(f[:, None].astype(np.int64) - 1 + np.arange(4)[None, :], 0, n_in - 1)
        return idx, cubic64(r - f)
    iy, wy = axis(h, H)
    ix, wx = axis(w, W)
    rows = (d[:, ix] * wx[None]).sum(-1)                                     # [h, W]
    return (rows[iy] * wy[:, :, None]).sum(1)                                # [H, W]


def tail64(depth, H, W):
    """(bytes, allowance mask) per sample."""
    outs, near = [], []
    for d in depth.double().numpy():
        r = resize64(d, H, W)
        rng = r.max() - r.min()
        v = (r - r.min()) / rng * 255.0 if rng > 0 else np.zeros_like(r)
        outs.append(np.clip(v, 0, 255).astype(np.uint8))
        near.append(np.abs(v - np.round(v)) < 1e-3)
    return np.stack(outs), np.stack(near)


def compare_bytes(tag, got, want, near):
    d = got.astype(np.int64) - want.astype(np.int64)
    bad = (d != 0) & ~(near & (np.abs(d) == 1))
    used = float(((d != 0) & near).mean())
    print(f"{tag}: {int((d != 0).sum())} of {d.size} bytes differ, all inside the allowance: {not bad.any()}; allowance used by {used:.4%}")
    assert not bad.any(), (tag, int(bad.sum()))
    assert used <= 0.01, (tag, used)


def tail_inputs():
    y, x = torch.meshgrid(torch.arange(12.0), torch.arange(10.0), indexing="ij")
    ramp = 3.0 * y + 0.37 * x
    step = (x >= 5).float() * 7.0 + 1.0
    noise = torch.randn(12, 10, generator=torch.Generator().manual_seed(20)).abs() * 50.0
    return torch.stack([ramp, step, noise])


@pytest.mark.parametrize("size", [(40, 40), (37, 50)])
def test_depth_tail(dev, size):
    H, W = size
    depth = tail_inputs()
    want, near = tail64(depth, H, W)
    # the inputs are fit for the comparison: torch's own fp32 result on the CPU stays inside the allowance and the cap
    r = F.interpolate(depth[:, None], size=(H, W), mode="bicubic", align_corners=False)
    mn, mx = torch.amin(r, dim=[1, 2, 3], keepdim=True), torch.amax(r, dim=[1, 2, 3], keepdim=True)
    t32 = (((r - mn) / (mx - mn))[:, 0].numpy() * 255.0).clip(0, 255).astype(np.uint8)
    compare_bytes(f"torch fp32 {size}", t32, want, near)
    flat, out = canary_out((3, H, W, 3), torch.uint8, dev, value=77)
    ops.depth_tail(depth.to(dev), (H, W), out=out)
    assert bool((flat[out.numel():] == 77).all())
    got = out.cpu().numpy()
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    compare_bytes(f"hip {size}", got[..., 0], want, near)
    # the step edge overshoots: the resized minimum lies below the input's, so the flat low side is not byte 0
    assert r[1].min().item() < depth[1].min().item() and got[1, 0, 0, 0] > 0
    assert got.min() == 0 and got.max() == 255


def test_depth_tail_constant_and_upscale(dev):
    """A constant map gives zeros (the reference divides 0 by 0 there); a 2048-pixel-block boundary: 64 x 64 -> 4096 pixels, 2 blocks."""
    out = ops.depth_tail(torch.full((1, 5, 7), 3.25, device=dev), (9, 11))
    assert int(out.max()) == 0
    depth = tail_inputs()[2:3]
    want, near = tail64(depth, 64, 64)
    compare_bytes("hip 64x64", ops.depth_tail(depth.to(dev), (64, 64)).cpu().numpy()[..., 0], want, near)
    # batch invariance: sample 1 of a batch against the same map alone
    two = torch.stack([tail_inputs()[0], tail_inputs()[2]]).to(dev)
    assert torch.equal(ops.depth_tail(two, (64, 64))[1], ops.depth_tail(two[1:].contiguous(), (64, 64))[0])
