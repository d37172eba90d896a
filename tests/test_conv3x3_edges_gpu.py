"""The three kernels of csrc/effvit.hip that five models share (conv3x3_kernel behind omg_conv3x3_nhwc_act / omg_conv3x3_nhwc_ex,
dwconv3x3_kernel, upsample_add_kernel) at their edges, bounded by a rounding model instead of a per-case tolerance (-m gpu).

References and case lists: tests/_conv3x3_model.py (CPU, on the STORED 16-bit operands).  tests/test_conv3x3_model.py shows without a
GPU that the checks below reject a kernel with any one of seventeen faults, at these very shapes.

The rule, elementwise, no element excluded:

    |out - truth|  <=  ulp16(truth) / 2  +  4 * E32  [+ 2^-20 |p| per tanh-GELU]

`truth` is float64; E32 = max |ref32 - truth| over the case (torch's fp32 evaluation on the CPU), floored at 2^-23 max |truth|; p is
the float64 pre-activation (the input, for gelu_in).  E32 and the activation allowance come from the CPU references and from the
derivation in tests/_conv3x3_model.py, not from the kernels: nothing here was fitted to what the GPU returned.

1. Dense kernel, both entries.  (Cin, Cout) in M.PAIRS: Cin 1, 2, 5, 7 (element loads), 8 (KV = 9: a last chunk of one vector), 24,
   40 (KV = 45), 256, 768; Cout 8, 40 (partial NT = 1 / 2 tiles), 72, 128 (one NT = 4 tile), 136, 200, 256 (a second tile, n0 = 128),
   264 (a third).  Pixels 1 x 1, 1 x 6, 6 x 1, 2 x 2, 7 x 9, 8 x 6, 3 images of 7 x 9, M = 127 / 128 / 129; stride 1 and 2, `same`
   on and off; bias, act 0 / 1 / 2, residual, relu_in taken in turn.  Families plain and offset (x = 100 + randn / 4, zero-mean
   weights).  Every call writes into a canary frame.  (a) the rule; (b) bit-exact integers at every (Cin, Cout, stride, same), odd
   and even extents; (c) each image of a batch of three between images of 1000s equals its single-image call bit for bit.
2. Depthwise kernel through out=: C 8, 24, 264, B = 3, input and output column slices of canary-filled buffers; without GELU equal
   to dwconv3x3_emulation bit for bit, with gelu / gelu_in / both under the rule; batch invariance.
3. Bicubic upsample-add at non-integer, non-square, identity, all-clamped, downscaling and 8x resizes, C 8 and 264: the rule; the
   identity size returns x (accumulate off) or round16(x + y0) bit for bit; a constant image returns the constant at every ratio.
4. Refusals: an error status and an untouched canary-filled output.

MEASURED (MI355X; the digest this module prints when it ends; with OMG_CONV3X3_ERRORS_JSON=path every case's figures go to that file)
A 16-bit output does not show the kernel's fp32 value, so the kernel's error over E32 is measured from below: `excess` is the error
beyond the half ulp of the one rounding to the storage type (for the GELU cases it still contains the activation's share).
1264 cases of the rule; worst of each kernel and type, with the case that gave it
kernel    type | cases | error / bound | excess / E32
dense     fp16 |   496 |        0.9986 |        0.501   (offset 5->200 3x1x43 s2 relu_in res | offset 256->264 1x8x6 s1 GELU res)
dense     bf16 |   496 |        0.9998 |        0.775   (plain 1->8 3x1x43 s1 relu_in res | offset 256->264 2x8x8 s2 GELU)
depthwise fp16 |   108 |        0.9969 |        0.199   (gelu_in C264 3x6x1 s1 | gelu_in C264 3x7x9 s1)
depthwise bf16 |   108 |        0.9995 |        0.107   (gelu_in C264 3x6x1 s1 | gelu_in C264 3x8x6 s2)
bicubic   fp16 |    28 |        0.9986 |        0.448   (accumulate 6x6->6x6 C264 | 7x5->9x8 C264)
bicubic   bf16 |    28 |        0.9999 |        0.445   (accumulate 6x6->6x6 C8 | 7x5->9x8 C264)
The error comes near the bound only where it is the half ulp of the one rounding (a result that lies next to a rounding boundary);
of the 4 E32 the rule grants, the kernels use at most 0.78.  The share of elements that are not round16(truth) is below 1 % except
in the offset family (15 % in fp16, 4 % in bf16), where cancellation makes E32 large against the result's ulp, as it is meant to.
The exact, bitwise, batch, canary and refusal tests passed as written: no kernel fault was found, effvit.hip is unchanged.
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from tests import _conv3x3_model as M

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
CANARY = -1234.0                # exact in fp16, -1232 in bf16: a frame is compared with itself, bit for bit
PAD = 64                        # canary elements in front of and behind a dense output (128 bytes: the views stay 16-byte aligned)

CASES = []                      # one record per case of the rule (M.held)


def _id(v):
    if isinstance(v, torch.dtype):
        return M.name(v)
    return "-".join(str(i) for i in v) if isinstance(v, tuple) else None


@pytest.fixture(scope="module", autouse=True)
def digest():
    yield
    print_digest()


def print_digest():
    if not CASES:
        return
    groups = {}
    for c in CASES:
        groups.setdefault((" ".join(c["tag"].split()[:2]), c["dtype"]), []).append(c)
    print(f"\n{len(CASES)} cases of the rule; worst of each group")
    print("group              type | cases | excess / E32 | error / bound | not round16(truth)")
    for key in sorted(groups):
        g = groups[key]
        print(f"{key[0]:18s} {key[1]} | {len(g):5d} | {max(c['excess_over_E32'] for c in g):12.2f} | {max(c['err_over_bound'] for c in g):13.2f} | "
              f"{max(c['not_round_truth'] for c in g):.4f}")
    path = os.environ.get("OMG_CONV3X3_ERRORS_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(CASES, f, indent=1)


def bits(t):
    return t.contiguous().view(torch.int16)


def framed_flat(shape, dtype, dev):
    """A contiguous view of `shape` with PAD canaries in front of it and behind it."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device=dev)
    return flat, flat[PAD:PAD + n].view(shape)


def flat_untouched(flat):
    n = flat.numel() - 2 * PAD
    ends = torch.cat([flat[:PAD], flat[PAD + n:]])
    return torch.equal(bits(ends), bits(torch.full_like(ends, CANARY)))


def all_canary(t):
    return torch.equal(bits(t), bits(torch.full_like(t, CANARY)))


# ------------------------------------------------------------------------------------------------------------------ 1. the dense kernel
def conv(dev, entry, x, w, bias, res, stride=1, act=0, relu_in=False, same=False):
    """One call with everything guarded; returns the output rows [M, Cout] on the CPU."""
    B, H, W, _ = x.shape
    shape = (B, M.out_size(H, stride), M.out_size(W, stride), w.shape[0])
    flat, view = framed_flat(shape, x.dtype, dev)
    xd, wd = x.to(dev), w.to(dev)
    bd, rd = None if bias is None else bias.to(dev), None if res is None else res.to(dev)
    if entry == "act":
        assert act in (0, 1) and not relu_in and not same
        out = ops.conv3x3_nhwc_act(xd, wd, stride=stride, bias=bd, gelu=bool(act), residual=rd, out=view)
    else:
        out = ops.conv3x3_nhwc_ex(xd, wd, stride=stride, bias=bd, act=act, residual=rd, relu_in=relu_in, same=same, out=view)
    assert out.data_ptr() == view.data_ptr()
    assert flat_untouched(flat), "wrote in front of or behind the output"
    assert torch.equal(bits(xd.cpu()), bits(x)) and torch.equal(bits(wd.cpu()), bits(w)), "an operand was written"
    return out.cpu().reshape(-1, shape[3])


def run_dense_cases(dev, dtype, pair, family):
    for n, c in enumerate(M.dense_cases(pair, family)):
        x, w, bias, res = M.dense_inputs(c, dtype, seed=n)
        kw = M.dense_kwargs(c)
        out = conv(dev, c.entry, x, w, bias, res, **kw)
        truth, allow = M.dense_truth(x, w, bias, res, **kw)
        M.held(M.dense_tag(c), dtype, out, truth, M.dense_ref32(x, w, bias, res, **kw), log=CASES, allow=allow)
        if c.entry == "act":                                                 # the other entry runs the same kernel: the same bits
            assert torch.equal(bits(conv(dev, "ex", x, w, bias, res, **kw)), bits(out)), M.dense_tag(c)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("pair", M.PAIRS, ids=_id)
def test_dense_holds_the_rule_at_every_edge(dev, dtype, pair):
    run_dense_cases(dev, dtype, pair, "plain")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("pair", M.OFFSET_PAIRS, ids=_id)
def test_dense_holds_the_rule_under_cancellation(dev, dtype, pair):
    """x = 100 + randn / 4 against zero-mean weights: the partial sums are two orders of magnitude above the result, E32 matters."""
    run_dense_cases(dev, dtype, pair, "offset")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("pair", M.PAIRS, ids=_id)
def test_dense_is_exact_on_small_integers(dev, dtype, pair):
    cin, cout = pair
    for B, H, W in M.exact_pixels(pair):
        for stride, same in M.EXACT_MODES:
            x, w, b, r = M.dense_integers(cin, cout, B, H, W, stride)
            ref, _ = M.dense_truth(x, w, b, r, stride=stride, same=same)
            assert torch.equal(ref, ref.to(dtype).double()) and ref.abs().max() >= 8, "the case itself must be exactly representable"
            for entry in ("ex",) if same else ("act", "ex"):
                got = conv(dev, entry, x.to(dtype), w.to(dtype), b.to(dtype), r.to(dtype), stride=stride, same=same)
                wrong = got.double() != ref
                assert not bool(wrong.any()), (f"{cin}->{cout} {B}x{H}x{W} s{stride} same{int(same)} {entry}: {int(wrong.sum())} of {wrong.numel()} wrong, "
                                               f"first at (pixel, channel) {tuple(int(i) for i in wrong.nonzero()[0])}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("pair", [(5, 200), (8, 264), (40, 136), (256, 264)], ids=_id)
def test_dense_images_of_a_batch_do_not_see_each_other(dev, dtype, pair):
    H, W = 7, 9
    for stride, same in M.EXACT_MODES:
        c = M.Dense(pair[0], pair[1], 3, H, W, stride, same, True, 1, True, False, "ex", "plain")
        x, w, bias, res = M.dense_inputs(c, dtype, seed=77)
        kw = M.dense_kwargs(c)
        for i in range(3):
            loud = torch.full_like(x, 1000.0)
            loud[i] = x[i]
            together = conv(dev, "ex", loud, w, bias, res, **kw).reshape(3, -1)
            alone = conv(dev, "ex", x[i:i + 1], w, bias, res[i:i + 1], **kw).reshape(-1)
            assert torch.equal(bits(together[i]), bits(alone)), f"{pair} s{stride} same{int(same)}: image {i} differs alone and between two loud images"


# -------------------------------------------------------------------------------------------------------------- 2. the depthwise kernel
def dw(dev, x, taps, bias, B, H, W, stride, gelu=False, gelu_in=False):
    """Input and output as column slices (at column 8) of wider canary-filled buffers, the output with a canary row behind it."""
    rows, C = x.shape
    orows = B * M.out_size(H, stride) * M.out_size(W, stride)
    wide = torch.full((rows, C + 24), CANARY, dtype=x.dtype)
    wide[:, 8:8 + C] = x
    wide = wide.to(dev)
    frame = torch.full((orows + 1, C + 16), CANARY, dtype=x.dtype, device=dev)
    view = frame[:orows, 8:8 + C]
    assert wide.stride(0) > C and view.stride(0) > C and view.stride(0) != wide.stride(0)
    out = ops.dwconv3x3_act(wide[:, 8:8 + C], taps.to(dev), B, H, W, stride=stride, bias=None if bias is None else bias.to(dev), gelu=gelu,
                            gelu_in=gelu_in, out=view)
    assert out.data_ptr() == view.data_ptr() and out.shape == (orows, C)
    assert all_canary(frame[:, :8]) and all_canary(frame[:, 8 + C:]) and all_canary(frame[orows:]), "wrote outside its column slice or behind the last pixel"
    assert all_canary(wide[:, :8]) and all_canary(wide[:, 8 + C:]) and torch.equal(bits(wide[:, 8:8 + C].cpu()), bits(x)), "the input buffer was written"
    return out.cpu().contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("C", M.DW_CHANNELS)
def test_depthwise_equals_its_emulation_bit_for_bit(dev, dtype, C):
    for n, (B, H, W) in enumerate(M.DW_PIXELS):
        for stride in (1, 2):
            x, taps, bias = M.dwconv_inputs(B, H, W, C, 3, dtype, seed=100 * C + 2 * n + stride)
            for b in (bias, None):
                got = dw(dev, x, taps, b, B, H, W, stride)
                want = M.dwconv3x3_emulation(x, taps, b, B, H, W, stride).to(dtype)
                same = bits(got) == bits(want)
                assert bool(same.all()), (f"C{C} {B}x{H}x{W} s{stride} bias {b is not None}: {int((~same).sum())} of {same.numel()} differ, "
                                          f"max |d| {float((got.float() - want.float()).abs().max()):.3e}")
            dense = ops.dwconv3x3_act(x.to(dev), taps.to(dev), B, H, W, stride=stride, bias=bias.to(dev))       # the default path: its own output
            assert dense.is_contiguous() and torch.equal(bits(dense.cpu()), bits(dw(dev, x, taps, bias, B, H, W, stride)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("C", M.DW_CHANNELS)
@pytest.mark.parametrize("gelu,gelu_in", [(True, False), (False, True), (True, True)])
def test_depthwise_with_gelu_holds_the_rule(dev, dtype, C, gelu, gelu_in):
    for n, (B, H, W) in enumerate(M.DW_PIXELS):
        for stride in (1, 2):
            x, taps, bias = M.dwconv_inputs(B, H, W, C, 3, dtype, seed=100 * C + 2 * n + stride, with_bias=bool((n + stride) % 2))
            got = dw(dev, x, taps, bias, B, H, W, stride, gelu, gelu_in)
            truth, allow = M.dw_truth(x, taps, bias, B, H, W, stride, gelu, gelu_in)
            M.held(f"dw gelu{int(gelu)}in{int(gelu_in)} C{C} {B}x{H}x{W} s{stride} bias{int(bias is not None)}", dtype, got, truth,
                   M.dw_ref32(x, taps, bias, B, H, W, stride, gelu, gelu_in), log=CASES, allow=allow)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("C", M.DW_CHANNELS)
def test_depthwise_images_of_a_batch_do_not_see_each_other(dev, dtype, C):
    for H, W in [(2, 2), (7, 9), (8, 6)]:
        for stride in (1, 2):
            x, taps, bias = M.dwconv_inputs(3, H, W, C, 3, dtype, seed=C + H)
            n = M.out_size(H, stride) * M.out_size(W, stride)
            for i in range(3):
                loud = torch.full_like(x, 1000.0)
                loud[i * H * W:(i + 1) * H * W] = x[i * H * W:(i + 1) * H * W]
                together = dw(dev, loud, taps, bias, 3, H, W, stride, gelu=True)
                alone = dw(dev, x[i * H * W:(i + 1) * H * W], taps, bias, 1, H, W, stride, gelu=True)
                assert torch.equal(bits(together[i * n:(i + 1) * n]), bits(alone)), f"C{C} {H}x{W} s{stride}: image {i}"


def test_depthwise_out_argument_is_checked(dev):
    x, taps, _ = M.dwconv_inputs(1, 4, 4, 16, 3, F16, seed=1)
    x, taps = x.to(dev), taps.to(dev)
    for bad in (torch.empty(16, 8, dtype=F16, device=dev), torch.empty(15, 16, dtype=F16, device=dev), torch.empty(16, 16, dtype=BF16, device=dev),
                torch.empty(16, 36, dtype=F16, device=dev)[:, :16], torch.empty(16, 32, dtype=F16, device=dev)[:, ::2], torch.empty(16, 16, dtype=F16),
                torch.empty(1, 16, 16, dtype=F16, device=dev)):
        with pytest.raises(AssertionError):
            ops.dwconv3x3_act(x, taps, 1, 4, 4, out=bad)
    with pytest.raises(AssertionError, match="overlaps"):
        ops.dwconv3x3_act(x, taps, 1, 4, 4, out=x)


# ------------------------------------------------------------------------------------------------------------------ 3. bicubic upsample
def up(dev, x, y0, accumulate):
    flat, view = framed_flat(tuple(y0.shape), x.dtype, dev)
    view.copy_(y0.to(dev))
    xd = x.to(dev)
    out = ops.upsample_add_nhwc(xd, view, accumulate=accumulate)
    assert out.data_ptr() == view.data_ptr()
    assert flat_untouched(flat), "wrote in front of or behind the output"
    assert torch.equal(bits(xd.cpu()), bits(x)), "the input was written"
    return out.cpu().reshape(-1, x.shape[3])


RESIZE_IDS = [f"{a}x{b}to{c}x{d}" for (a, b), (c, d) in M.RESIZES]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("resize", M.RESIZES, ids=RESIZE_IDS)
def test_upsample_add_holds_the_rule(dev, dtype, resize):
    (hin, win), (hout, wout) = resize
    B = 2
    for C in M.UP_CHANNELS:
        x, y0 = M.up_inputs(B, hin, win, hout, wout, C, dtype, seed=hin + wout + C)
        for acc in (False, True):
            got = up(dev, x, y0, acc)
            M.held(f"up acc{int(acc)} {hin}x{win}->{hout}x{wout} C{C}", dtype, got, M.up_truth(x, hout, wout, y0, acc), M.up_ref32(x, hout, wout, y0, acc),
                   log=CASES)
            if (hin, win) == (hout, wout):                                   # the weights are exactly (0, 1, 0, 0) in fp32
                want = (x.double() + y0.double()).to(torch.float32).to(dtype) if acc else x          # the kernel adds in fp32, then stores
                assert torch.equal(bits(got), bits(want.reshape(-1, C))), f"identity size, accumulate {acc}"


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("resize", M.RESIZES, ids=RESIZE_IDS)
def test_upsample_of_a_constant_image_is_that_constant(dev, dtype, resize):
    (hin, win), (hout, wout) = resize
    for C, value in zip(M.UP_CHANNELS, (-3.3125, 0.00390625)):
        x = torch.full((2, hin, win, C), value).to(dtype)
        assert float(x[0, 0, 0, 0]) == value, "a value of the 16-bit grid"
        got = up(dev, x, torch.zeros(2, hout, wout, C, dtype=dtype), False)
        assert torch.equal(bits(got), bits(torch.full_like(got, value)))


# ------------------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_output_untouched(dev):
    """What tests/test_effvit.py and tests/test_dpt.py check with stand-in addresses, on real buffers: an error status, no launch."""
    lib = L.lib()
    f16 = L.OMG_F16
    buf = lambda n: torch.zeros(n, dtype=F16, device=dev)                                    # noqa: E731
    x, w, y = buf(8 * 8 * 32 + 8), buf(32 * 9 * 32), torch.full((8 * 8 * 64,), CANARY, dtype=F16, device=dev)
    X, Wt, Y = x.data_ptr(), w.data_ptr(), y.data_ptr()

    def act(Cin=32, Cout=32, stride=1, a=0, X=X):
        return lib.omg_conv3x3_nhwc_act(f16, X, 1, 8, 8, Cin, Cout, stride, Wt, None, a, None, Y, None)

    def ex(Cin=32, Cout=32, stride=1, a=0, flags=0, X=X):
        return lib.omg_conv3x3_nhwc_ex(f16, X, 1, 8, 8, Cin, Cout, stride, Wt, None, a, None, flags, Y, None)

    def dwc(C=32, ldx=32, ldy=32):
        return lib.omg_dwconv3x3_act(f16, X, ldx, 1, 8, 8, C, 1, Wt, None, 0, Y, ldy, None)

    for call in (lambda: act(Cin=12), lambda: ex(Cin=12), lambda: act(Cout=12), lambda: ex(Cout=12), lambda: act(stride=3), lambda: ex(stride=3),
                 lambda: act(a=2), lambda: ex(a=3), lambda: ex(flags=4), lambda: act(X=X + 8), lambda: ex(X=X + 8),
                 lambda: dwc(ldy=24), lambda: dwc(ldy=36), lambda: dwc(ldx=24), lambda: dwc(C=12, ldx=16, ldy=16)):
        assert call() == -1                                                  # OMG_EINVAL; a failed launch would be -3
        assert lib.omg_last_error()
    torch.cuda.synchronize()
    assert all_canary(y), "a refused call wrote its output"
    assert act(Cin=4, X=X + 8) == 0 and ex(a=2, flags=3) == 0 and dwc(ldy=40) == 0      # and their accepted neighbours run
    torch.cuda.synchronize()
