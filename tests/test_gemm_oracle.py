"""tests/_gemm_oracle.py pinned without a GPU: every exact case of tests/test_gemm_tiles_gpu.py is representable in fp16 and bf16 and is no
degenerate matrix, the float64 references mean what ``ops.gemm`` / ``ops.conv2d`` document, and the rounding bound tells one rounding
from two."""
import pytest
import torch
import torch.nn.functional as F

from omg_amd import ops
from tests import _gemm_oracle as O


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("epi", O.LINEAR_EPILOGUES)
@pytest.mark.parametrize("name", list(O.CONV_CASES))
def test_exact_conv_case_is_representable_and_alive(name, epi):
    ref, S = O.conv_expected(name, "int", None, epi)          # asserts representability in both dtypes, max |ref| >= 8, < 1/4 zeros
    d = O.conv_case(name, "int")
    assert S is None and tuple(ref.shape) == d["out_shape"]
    for k in ("x1", "x2", "w"):
        if d[k] is not None:
            assert set(d[k].unique().tolist()) == {-1.0, 0.0, 1.0}, "a dead operand"
    assert float((d["w"] != 0).double().mean()) < 0.8, "w is sparse"
    for k in ("bias", "group_bias", "residual"):
        assert float(d[k].abs().max()) == 4 and torch.equal(d[k], d[k].round())
    # every partial sum is an integer the fp32 accumulator holds exactly, whatever the order: sum of |products| < 2^24
    assert float(O.conv_acc64(d["x1"].abs(), d["w"].abs(), d["ksize"], x2=None if d["x2"] is None else d["x2"].abs(), **d["geo"]).max()) + 8 < 2 ** 24


@pytest.mark.parametrize("name", list(O.GEMM_CASES))
def test_exact_gemm_case_is_representable_and_alive(name):
    d = O.gemm_case(name, "int")
    for epi in d["epis"]:
        ref, S = O.gemm_expected(name, "int", None, epi)
        assert S is None and tuple(ref.shape) == (O.GEMM_CASES[name]["M"], O.GEMM_CASES[name]["N"])
        if d["slots"]:
            rows = ref.shape[0] // d["groups"]
            for g, ad in enumerate(d["adapter"].tolist()):
                assert bool((ref[g * rows:(g + 1) * rows] == O.OUT_INIT).all()) == (ad < 0), "skipped groups, and only they, keep what was there"


def test_exact_cases_see_a_wrong_tap_a_wrong_channel_block_and_a_wrong_upsample_shift():
    """What the exact comparison is for: a kernel that reads one tap from the neighbouring pixel, takes the second input's channels from
    the first, or gets the upsample's ``>> 1`` wrong (here: source row (y + 1) >> 1 for y >> 1) differs from the reference by at least
    1/2 on many outputs."""
    d = O.conv_case("up", "int")
    ref, _ = O.conv_expected("up", "int", None, "residual")
    e = O.conv_epi_args(d, "residual")
    w = d["w"].view(O.COUT, 3, 3, 128)
    wrong_tap = torch.roll(w, 1, dims=2).reshape(O.COUT, -1)
    wrong_x2 = torch.cat([d["x1"], d["x1"]], dim=-1)
    doubled = torch.cat([d["x1"], d["x2"]], dim=-1).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(O.conv2d_ref64(doubled, d["w"], 3, **e), ref), "the pre-doubled input is the fused upsample"
    wrong_shift = torch.roll(doubled, -1, dims=1)          # row y of the doubled image now holds source row (y + 1) >> 1
    for what, got in (("tap", O.conv2d_ref64(d["x1"], wrong_tap, 3, x2=d["x2"], **d["geo"], **e)),
                      ("x2", O.conv2d_ref64(wrong_x2, d["w"], 3, **d["geo"], **e)),
                      ("upsample shift", O.conv2d_ref64(wrong_shift, d["w"], 3, **e))):
        diff = (got - ref).abs()
        assert float(diff[diff > 0].min()) >= 0.5 and float((diff > 0).double().mean()) > 0.5, what


# ------------------------------------------------------------------------------------------------ the references
def test_conv_reference_is_the_documented_convolution():
    """Packed weight order (tap row, tap column, channel) = ops.pack_conv_weight; nearest upsample = F.interpolate; concat = torch.cat."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(16, 24, 3, 3, generator=g, dtype=torch.float64)
    assert torch.equal(O.unpack_conv_weight(ops.pack_conv_weight(w), 3), w)
    x1, x2 = torch.randn(2, 5, 4, 16, generator=g, dtype=torch.float64), torch.randn(2, 5, 4, 8, generator=g, dtype=torch.float64)
    b, gb = torch.randn(16, generator=g, dtype=torch.float64), torch.randn(2, 16, generator=g, dtype=torch.float64)
    res = torch.randn(2, 10, 8, 16, generator=g, dtype=torch.float64)
    got = O.conv2d_ref64(x1, ops.pack_conv_weight(w), 3, upsample=True, x2=x2, bias=b, group_bias=gb, residual=res, out_scale=0.5)
    x = F.interpolate(torch.cat([x1, x2], -1).permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    want = (F.conv2d(x, w, b, padding=1) + gb[:, :, None, None]) * 0.5 + res.permute(0, 3, 1, 2)
    torch.testing.assert_close(got.permute(0, 3, 1, 2), want, rtol=1e-13, atol=1e-13)
    # stride 2 on an odd and an even image: output pixel (y, x) is centred on input pixel (2 y, 2 x)
    for H in (5, 6):
        xs = torch.randn(1, H, H, 8, generator=g, dtype=torch.float64)
        w1 = torch.randn(4, 8, 1, 1, generator=g, dtype=torch.float64)
        got = O.conv2d_ref64(xs, ops.pack_conv_weight(w1), 1, stride=2)
        torch.testing.assert_close(got, xs[:, ::2, ::2] @ w1[:, :, 0, 0].T, rtol=1e-13, atol=1e-13)


def test_gemm_reference_is_the_documented_gemm():
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    a, w3, b, gb, res = r(12, 16), r(2, 8, 16), r(8), r(3, 8), r(12, 8)
    init = r(12, 8)
    ad = torch.tensor([1, -1, 0], dtype=torch.int32)
    got = O.gemm_ref64(a, w3, bias=b, group_bias=gb, groups=3, out_scale=2.0, residual=res, adapter=ad, out_init=init)
    torch.testing.assert_close(got[0:4], (a[0:4] @ w3[1].T + b + gb[0]) * 2 + res[0:4], rtol=1e-13, atol=1e-13)
    assert torch.equal(got[4:8], init[4:8])
    torch.testing.assert_close(got[8:12], (a[8:12] @ w3[0].T + b + gb[2]) * 2 + res[8:12], rtol=1e-13, atol=1e-13)
    # the second K-segment: added where the adapter is >= 0; a shared (2-D) weight computes the base for every group
    a2, w2 = r(12, 8), r(2, 8, 8)
    got = O.gemm_ref64(a, w3[0], groups=3, adapter=ad, a2=a2, w2=w2, act="silu")
    torch.testing.assert_close(got[0:4], F.silu(a[0:4] @ w3[0].T + a2[0:4] @ w2[1].T), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(got[4:8], F.silu(a[4:8] @ w3[0].T), rtol=1e-13, atol=1e-13)
    # GEGLU on the packed rows = value * gelu(gate) of the plain halves
    wp, bp = r(128, 16), r(128)
    perm = ops.geglu_row_perm(128)
    got = O.gemm_ref64(a, wp[perm], bias=bp[perm], act="geglu", out_scale=2.0)
    val, gate = (a @ wp.T + bp).chunk(2, dim=-1)
    torch.testing.assert_close(got, val * F.gelu(gate) * 2, rtol=1e-13, atol=1e-13)


# ------------------------------------------------------------------------------------------------ the rounding bound
@pytest.mark.parametrize("dtype", O.DTYPES)
def test_ulp_is_the_spacing_of_the_format(dtype):
    p, e_min = O.FMT[dtype]
    x = torch.tensor([0.0, 2.0 ** (e_min - 3), 2.0 ** e_min, 0.99, 1.0, 1.5, 2.0 - 2.0 ** -20, 2.0, 100.0, -3.0], dtype=torch.float64)
    want = torch.tensor([e_min, e_min, e_min, -1, 0, 0, 0, 1, 6, 1], dtype=torch.float64)
    assert torch.equal(O.ulp(x, dtype), 2.0 ** (want - p))
    # against the format itself: the gap to the next representable number
    y = torch.tensor([1.0, 3.0, 100.0, 0.007], dtype=dtype)
    nxt = (y.view(torch.int16) + 1).view(dtype)
    assert torch.equal(O.ulp(y.double(), dtype), nxt.double() - y.double())


def _bound_accepts_one_rounding_and_rejects_two(ref, S, pre, twice, K, dtype, what, blind):
    """The rounding too many errs at most half an ulp of ``pre``, the value it rounds.  The bound must refuse the twice-rounded result
    somewhere, unless the case is listed as blind; and a case is listed as blind only for the stated reason: its accumulation term
    (K + 4) 2^-23 S is at least that half ulp on every output."""
    tol = O.bound(ref, S, K, 0, dtype)
    once = (O.round16(ref, dtype) - ref).abs()
    assert bool((once <= tol).all()), f"{what}: the bound refuses the correctly rounded result"
    bad = ((twice - ref).abs() > tol).double().mean().item()
    swamped = ((K + 4) * 2.0 ** -23 * S >= 0.5 * O.ulp(pre, dtype)).double().mean().item()
    print(f"{what} {dtype}: the twice-rounded result breaks the bound on {bad:.2%} of the elements; the accumulation term is at least "
          f"the second rounding's half ulp on {swamped:.2%}")
    if blind:
        assert swamped == 1.0, f"{what}: listed as blind, but the accumulation term is below half an ulp on {1 - swamped:.2%} of the outputs"
    else:
        assert bad > 0, f"{what}: the bound cannot tell one rounding from two"


@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("name", list(O.CONV_CASES))
def test_conv_bound_tells_one_rounding_from_two(name, dtype):
    ref, S = O.conv_expected(name, "rnd", dtype, "residual")
    pre, twice = O.conv_twice_rounded(name, dtype)
    _bound_accepts_one_rounding_and_rejects_two(ref, S, pre, twice, O.conv_case(name, "rnd", dtype)["K"], dtype, f"conv {name}",
                                                (name, dtype) in O.BLIND)
    for epi in ("bias", "group_bias"):
        ref, S = O.conv_expected(name, "rnd", dtype, epi)
        assert bool(((O.round16(ref, dtype) - ref).abs() <= O.bound(ref, S, 1, 0, dtype)).all())


def test_blind_cases_are_the_two_long_fp16_convolutions():
    assert O.BLIND == {(n, torch.float16) for n in O.CONV_CASES if O.conv_case(n, "rnd", torch.float16)["K"] > 576}


@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("name", ["layouts", "k72"])
def test_gemm_bound_tells_one_rounding_from_two(name, dtype):
    ref, S = O.gemm_expected(name, "rnd", dtype, "residual")
    pre, twice = O.gemm_twice_rounded(name, dtype)
    _bound_accepts_one_rounding_and_rejects_two(ref, S, pre, twice, O.GEMM_CASES[name]["K"], dtype, f"gemm {name}", False)
