"""The references of tests/_conv3x3_model.py, checked without a GPU: the unfaulted emulations of the three kernels of csrc/effvit.hip
hold the rule on the case lists tests/test_conv3x3_edges_gpu.py runs, the depthwise emulation rounds to round16(truth), the integer
generators are exact in both storage types, and every named fault is rejected at one of the GPU suite's own shapes: by the rule, by
the exact-integer comparison or by the bitwise depthwise comparison.  A fault that nothing catches fails here by name."""
import pytest
import torch

from tests import _conv3x3_model as M

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]


def _id(v):
    if isinstance(v, torch.dtype):
        return M.name(v)
    return f"{v[0]}-{v[1]}" if isinstance(v, tuple) else None


def bits(t):
    return t.contiguous().view(torch.int16)


def round16(t, dtype):
    """Round to nearest even on the grid of `dtype`, in float64 (a float64 -> 16-bit conversion may round twice)."""
    u = M.ulp16(t, dtype)
    return torch.round(t / u) * u


def rule(tag, dtype, c, x, w, bias, res, out32):
    truth, allow = M.dense_truth(x, w, bias, res, **M.dense_kwargs(c))
    return M.held(tag, dtype, out32.to(dtype), truth, M.dense_ref32(x, w, bias, res, **M.dense_kwargs(c)), allow=allow)


# ------------------------------------------------------------------------------------------------------------------------ the lists
def test_the_case_lists_cover_every_edge_the_suite_names():
    cases = [c for p in M.PAIRS for c in M.dense_cases(p)]
    assert {c.cin for c in cases} == {1, 2, 5, 7, 8, 24, 40, 256, 768} and {c.cout for c in cases} == {8, 40, 72, 128, 136, 200, 256, 264}
    assert {(768, 256), (256, 264), (5, 200)} <= set(M.PAIRS)
    for p in M.PAIRS:
        assert {(c.B, c.H, c.W) for c in M.dense_cases(p)} == set(M.BIG_PIXELS.get(p, M.PIXELS))
    ms = {c.B * c.H * c.W for c in cases if c.stride == 1}
    assert {1, 6, 4, 63, 48, 189, 127, 128, 129} <= ms
    assert max(c.B * c.H * c.W for c in cases if (c.cin, c.cout) == (768, 256)) == 2 * 9 * 7
    epi = lambda c: (c.bias, c.act, c.res, c.relu_in)                                       # noqa: E731
    assert {(epi(c), c.stride, c.same) for c in cases} >= {(e[:4], s, sm) for e in M.EPILOGUES for s, sm in M.MODES}
    assert {(c.entry, c.act) for c in cases} >= {("act", 0), ("act", 1), ("ex", 0), ("ex", 1), ("ex", 2)}
    assert all(c.entry == "ex" for c in cases if c.act == 2 or c.relu_in or c.same)
    assert {(c.cout, e) for c in cases for e in [epi(c)]} >= {(co, e[:4]) for co in (136, 200, 264) for e in M.EPILOGUES}   # in a second tile
    assert set(M.OFFSET_PAIRS) <= set(M.PAIRS)


# ------------------------------------------------------------------------------------------------------------------ the dense kernel
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("pair", M.PAIRS, ids=_id)
def test_the_unfaulted_dense_emulation_holds_the_rule_on_every_case(dtype, pair):
    worst = 0.0
    for family in ("plain", "offset") if pair in M.OFFSET_PAIRS else ("plain",):
        for n, c in enumerate(M.dense_cases(pair, family)):
            x, w, bias, res = M.dense_inputs(c, dtype, seed=n)
            rec = rule(M.dense_tag(c), dtype, c, x, w, bias, res, M.conv3x3_emulation(x, w, bias, res, **M.dense_kwargs(c)))
            worst = max(worst, rec["excess_over_E32"])
    print(f"{pair} {M.name(dtype)}: worst excess / E32 {worst:.2f}")


def _dense_fault_applies(fault, c):
    KV = 9 * ((c.cin + 7) // 8)
    return {"col_tile_offset": c.cout > 128, "drop_last_chunk": KV % 4 != 0, "wrap_row": c.W > 1 and c.H > 1 and not (c.same and c.stride == 2 and c.W % 2 == 0),      # no padding in front of an even width
            "wrap_batch": c.B > 1 and c.H > 1,
            "same_origin": c.same and c.stride == 2 and (c.H % 2 == 0 or c.W % 2 == 0), "stride_phase": c.stride == 2 and c.H * c.W > 1,
            "residual_before_act": c.res and c.act != 0, "relu_on_residual": c.res and c.relu_in, "cin_pad_garbage": c.cin < 8}[fault]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("fault", M.DENSE_FAULTS)
def test_the_rule_rejects_each_dense_fault(dtype, fault):
    """At the suite's own cases where the fault can act, the unfaulted emulation holds the rule and the faulted one breaks it: in
    every such case of three pairs with at least 6 x 6 pixels, not in one lucky one (in a single row or column a fault may meet
    nothing but padding)."""
    caught = total = missed_wide = 0
    for pair in [(5, 200), (8, 264), (40, 136)]:
        for n, c in enumerate(M.dense_cases(pair)):
            if not _dense_fault_applies(fault, c):
                continue
            x, w, bias, res = M.dense_inputs(c, dtype, seed=n)
            rule(M.dense_tag(c), dtype, c, x, w, bias, res, M.conv3x3_emulation(x, w, bias, res, **M.dense_kwargs(c)))
            total += 1
            try:
                rule(fault, dtype, c, x, w, bias, res, M.conv3x3_emulation(x, w, bias, res, fault=fault, **M.dense_kwargs(c)))
                missed_wide += c.H >= 6 and c.W >= 6
            except AssertionError:
                caught += 1
    print(f"{fault} {M.name(dtype)}: the rule rejects it in {caught} of {total} cases")
    assert caught >= 4 and missed_wide == 0, (fault, caught, total, missed_wide)


def _exact_case(pair, pixels, stride, same, dtype):
    B, H, W = pixels
    x, w, b, r = M.dense_integers(pair[0], pair[1], B, H, W, stride)
    kw = dict(stride=stride, same=same)
    ref, _ = M.dense_truth(x, w, b, r, **kw)
    return (x.to(dtype), w.to(dtype), b.to(dtype), r.to(dtype)), kw, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("pair", M.PAIRS + [(1024, 136)], ids=_id)
def test_the_integer_generator_is_exact_in_the_storage_type(dtype, pair):
    for pixels, (stride, same) in [(p, m) for p in M.exact_pixels(pair) for m in M.EXACT_MODES]:
        (x, w, b, r), kw, ref = _exact_case(pair, pixels, stride, same, dtype)
        again, _ = M.dense_truth(x, w, b, r, **kw)                                         # from the STORED operands: nothing was rounded
        assert torch.equal(again, ref)
        assert torch.equal(ref, ref.to(dtype).double()) and ref.abs().max() >= 8, "the case itself must be exactly representable"
        assert ref.abs().max() <= (2048 if dtype == F16 else 256)                           # every partial sum too: an integer of the type
        if pair[0] * pair[1] <= 40 * 264:
            assert torch.equal(M.conv3x3_emulation(x, w, b, r, **kw), ref)
        if pair[0] >= 8:                  # every (tap, cin) position carries weight in several output channels: no K position goes unseen
            assert int((w != 0).sum(0).min()) >= (8 if pair[1] >= 136 else 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("fault", [f for f in M.DENSE_FAULTS if f not in ("residual_before_act", "relu_on_residual")])
def test_the_exact_integer_comparison_rejects_each_dense_fault(dtype, fault):
    """No activation in the integer cases, so the two epilogue-order faults are the rule's alone."""
    caught = total = 0
    for pair in [(5, 200), (8, 264), (40, 136)]:
        for (B, H, W), (stride, same) in [(p, m) for p in M.exact_pixels(pair) for m in M.EXACT_MODES]:
            c = M.Dense(pair[0], pair[1], B, H, W, stride, same, True, 0, True, False, "ex", "integers")
            if not _dense_fault_applies(fault, c):
                continue
            (x, w, b, r), kw, ref = _exact_case(pair, (B, H, W), stride, same, dtype)
            total += 1
            caught += not torch.equal(M.conv3x3_emulation(x, w, b, r, fault=fault, **kw), ref)
    assert total >= 1 and caught == total, (fault, caught, total)


def test_batch_of_three_with_loud_neighbours_shows_a_wrapped_dense_tap():
    """The GPU test's form of the batch check: one image among two of 1000s against that image alone."""
    c = M.Dense(8, 72, 1, 7, 9, 1, False, True, 0, False, False, "act", "plain")
    x, w, bias, _ = M.dense_inputs(c, F16, seed=3)
    loud = torch.full_like(x, 1000.0)
    alone = M.conv3x3_emulation(x, w, bias)
    for i in range(3):
        batch = torch.cat([x if j == i else loud for j in range(3)])
        n = alone.shape[0]
        assert torch.equal(M.conv3x3_emulation(batch, w, bias)[i * n:(i + 1) * n], alone)
        assert not torch.equal(M.conv3x3_emulation(batch, w, bias, fault="wrap_batch")[i * n:(i + 1) * n], alone)
        assert not torch.equal(M.conv3x3_emulation(batch, w, bias, fault="wrap_row")[i * n:(i + 1) * n], alone) or i == 0


# -------------------------------------------------------------------------------------------------------------- the depthwise kernel
ACTS = [(False, False), (True, False), (False, True), (True, True)]


def dw_cases():
    return [(C, B, H, W, stride) for C in M.DW_CHANNELS for B, H, W in M.DW_PIXELS for stride in (1, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_the_unfaulted_depthwise_emulation_holds_the_rule_and_rounds_like_the_truth(dtype):
    """Without GELU the emulation's fp32 value is within 10 roundings of the float64 sum, |a32 - truth| <= 10 2^-24 (sum |x| |w| +
    |bias|), so that its rounding equals round16(truth) wherever truth is farther than that, plus 2^-30 relative, from a rounding
    boundary: everywhere but in a small share of the elements.  (2^-30 alone does not do: the fp32 chain is not exact, and a few fp16
    elements in ten thousand then round to the other side.)"""
    near = total = 0
    for n, (C, B, H, W, stride) in enumerate(dw_cases()):
        for with_bias in (True, False):
            x, taps, bias = M.dwconv_inputs(B, H, W, C, 3, dtype, seed=n, with_bias=with_bias)
            for gelu_out, gelu_in in ACTS:
                truth, allow = M.dw_truth(x, taps, bias, B, H, W, stride, gelu_out, gelu_in)
                a32 = M.dwconv3x3_emulation(x, taps, bias, B, H, W, stride, gelu_out=gelu_out, gelu_in=gelu_in)
                M.held(f"dw C{C} {B}x{H}x{W} s{stride} gelu{int(gelu_out)} gelu_in{int(gelu_in)}", dtype, a32.to(dtype), truth,
                       M.dw_ref32(x, taps, bias, B, H, W, stride, gelu_out, gelu_in), allow=allow)
                assert (allow is None) == (not gelu_out and not gelu_in)
            truth, _ = M.dw_truth(x, taps, bias, B, H, W, stride)
            a32 = M.dwconv3x3_emulation(x, taps, bias, B, H, W, stride)
            mag, _ = M.dw_truth(x.abs(), taps.abs(), None if bias is None else bias.abs(), B, H, W, stride)
            slack = 10 * 2.0 ** -24 * mag + 2.0 ** -30 * truth.abs()
            assert bool(((a32.double() - truth).abs() <= 10 * 2.0 ** -24 * mag).all())
            u = M.ulp16(truth, dtype)
            q = truth / u
            far = ((q - torch.floor(q) - 0.5).abs() * u > slack) & (M.ulp16(truth.abs() + u, dtype) == u)
            assert torch.equal(a32.to(dtype).double()[far], round16(truth, dtype)[far])
            near, total = near + int((~far).sum()), total + far.numel()
    print(f"{M.name(dtype)}: {near} of {total} elements are too near a rounding boundary to call")
    assert near < 0.02 * total


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_the_stride_1_depthwise_emulation_is_the_litemla_one(dtype):
    from tests._litemla_model import dwconv_emulation
    for C, B, H, W, _ in dw_cases()[::2]:
        x, taps, bias = M.dwconv_inputs(B, H, W, C, 3, dtype, seed=C + H)
        assert torch.equal(M.dwconv3x3_emulation(x, taps, bias, B, H, W, 1), dwconv_emulation(x, taps, bias, B, H, W, 3))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("fault", M.DW3_FAULTS)
def test_each_depthwise_fault_is_rejected(dtype, fault):
    """swap_ty_tx, wrap_batch and bias_after_round by the bitwise comparison, the padding fault (which needs gelu_in) by the rule."""
    caught = total = 0
    for n, (C, B, H, W, stride) in enumerate(dw_cases()):
        if C > 24 or (H, W) in ((1, 1),) or (fault == "wrap_batch" and H == 1):
            continue
        x, taps, bias = M.dwconv_inputs(B, H, W, C, 3, dtype, seed=n)
        total += 1
        if fault == "gelu_in_on_padding_as_nonzero":
            truth, allow = M.dw_truth(x, taps, bias, B, H, W, stride, False, True)
            ref32 = M.dw_ref32(x, taps, bias, B, H, W, stride, False, True)
            M.held("good", dtype, M.dwconv3x3_emulation(x, taps, bias, B, H, W, stride, gelu_in=True).to(dtype), truth, ref32, allow=allow)
            try:
                M.held(fault, dtype, M.dwconv3x3_emulation(x, taps, bias, B, H, W, stride, fault=fault, gelu_in=True).to(dtype), truth, ref32, allow=allow)
            except AssertionError:
                caught += 1
        else:
            good = M.dwconv3x3_emulation(x, taps, bias, B, H, W, stride).to(dtype)
            bad = M.dwconv3x3_emulation(x, taps, bias, B, H, W, stride, fault=fault).to(dtype)
            caught += not torch.equal(bits(good), bits(bad))
    assert total >= 8 and caught == total, (fault, caught, total)


# ------------------------------------------------------------------------------------------------------------------ bicubic upsample
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("resize", M.RESIZES, ids=lambda r: f"{r[0][0]}x{r[0][1]}to{r[1][0]}x{r[1][1]}")
def test_the_unfaulted_bicubic_emulation_holds_the_rule(dtype, resize):
    (hin, win), (hout, wout) = resize
    B = 2
    for C in M.UP_CHANNELS:
        x, y0 = M.up_inputs(B, hin, win, hout, wout, C, dtype, seed=hin + wout + C)
        for acc in (False, True):
            M.held(f"up {resize} C{C} acc{int(acc)}", dtype, M.upsample_emulation(x, hout, wout, y0, acc).to(dtype),
                   M.up_truth(x, hout, wout, y0, acc), M.up_ref32(x, hout, wout, y0, acc))
        if (hin, win) == (hout, wout):                                      # the weights are exactly (0, 1, 0, 0)
            assert torch.equal(bits(M.upsample_emulation(x, hout, wout).to(dtype)), bits(x.reshape(-1, C)))
            assert torch.equal(M.upsample_emulation(x, hout, wout, y0, True), x.double().reshape(-1, C) + y0.double().reshape(-1, C))
        const = torch.full_like(x, -3.3125)
        assert bool((M.upsample_emulation(const, hout, wout).to(dtype) == const[0, 0, 0, 0]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("fault", M.UP_FAULTS)
def test_the_rule_rejects_each_bicubic_fault(dtype, fault):
    caught = []
    for (hin, win), (hout, wout) in M.RESIZES:
        x, y0 = M.up_inputs(2, hin, win, hout, wout, 8, dtype, seed=hin + wout)
        truth, ref32 = M.up_truth(x, hout, wout), M.up_ref32(x, hout, wout)
        try:
            M.held(fault, dtype, M.upsample_emulation(x, hout, wout, fault=fault).to(dtype), truth, ref32)
        except AssertionError:
            caught.append(((hin, win), (hout, wout)))
    print(f"{fault} {M.name(dtype)}: rejected at {caught}")
    identity = ((6, 6), (6, 6))
    assert identity not in caught                        # weights (0, 1, 0, 0) and source = destination there: no fault can show
    want = {"swapped_scales": [((5, 7), (8, 9)), ((7, 5), (9, 8))]}.get(fault, [r for r in M.RESIZES if r != identity])
    assert all(r in caught for r in want), (fault, caught)


def test_the_activation_allowance_is_the_derived_one():
    assert M.ALLOW == 2.0 ** -20 and 1.12 < M.GELU_SLOPE < 1.13
    x = torch.linspace(-12, 12, 48001)
    z = 1.5957691216057308 * x.double() * (1 + 0.044715 * x.double() ** 2)
    s = torch.sigmoid(z)
    assert float((z * s * (1 - s)).abs().max()) <= 0.2245                              # the step of the derivation that bounds the argument's share
    assert bool(((M.gelu_f32(x).double() - M.gelu(x.double())).abs() <= M.ALLOW * x.double().abs()).all())     # and the host's fp32 evaluation fits
