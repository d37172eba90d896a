"""The yardstick of the MX-fp8 tests, oracle/mx8.py, checked on the CPU against its written contract in exact arithmetic —
before tests/test_mx8_quantisers_gpu.py compares the HIP quantisers with it byte for byte.

* scale rule: for EVERY positive finite fp16 / bf16 pattern as a block's amax, the smallest e >= -127 with amax <= 448 * 2^e
  (float64 comparisons of exact values);
* no finite input produces an e4m3 NaN byte; dequantize(quantize(x)) is within half an e4m3 ulp at the block's scale;
* sign of zero: an underflowed negative is 0x80, a positive 0x00 (torch's float8_e4m3fn cast, which the device must match);
* non-finite input: the contract of the module docstring, with the mask of unspecified blocks.
"""
import numpy as np
import pytest
import torch

from oracle import mx8
from tests import _mx8_patterns as P

DTYPES = [torch.float16, torch.bfloat16]
TOP = {torch.float16: 0x7bff, torch.bfloat16: 0x7f7f}


def _amax_blocks(dtype):
    """Every positive finite pattern as the only non-zero element of a block, position rotating: fp32 [rows, 128], patterns."""
    pats = np.arange(1, TOP[dtype] + 1, dtype=np.uint16)
    blocks = np.zeros((len(pats), 32), dtype=np.uint16)
    blocks[np.arange(len(pats)), np.arange(len(pats)) % 32] = pats
    return P.to_float(P.rows_of(blocks), dtype), pats


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_rule_on_every_amax_pattern(dtype):
    x, pats = _amax_blocks(dtype)
    ex = mx8.block_exponents(x).reshape(-1)[:len(pats)].to(torch.float64)
    amax = P.to_float(pats, dtype).to(torch.float64)                  # exact
    bound = 448.0 * torch.pow(torch.tensor(2.0, dtype=torch.float64), ex)     # exact: 448 * 2^e >= 2^-119
    assert (ex >= -127).all()
    assert (amax <= bound).all(), "a block saturates"
    smaller = (ex > -127) & (amax <= bound / 2)
    assert not smaller.any(), f"not the smallest scale: first amax pattern 0x{int(pats[int(smaller.nonzero()[0])]):04x}"
    assert (int(ex.min()), int(ex.max())) == ((-32, 8) if dtype == torch.float16 else (-127, 120))
    assert int((ex == -127).sum()) == (0 if dtype == torch.float16 else 1120)      # amax <= 448 * 2^-127
    # the patterns helper restates the same contract pattern by pattern
    for p_ in (1, 2, 1120, 1121, P.TINY_BF16_LAST, P.TINY_BF16_LAST + 1, TOP[dtype]):
        assert P.scale_exponent(p_, dtype) == int(ex[p_ - 1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_form_of_the_scale_rule(dtype):
    """mx8_scale_exp (omg_amd/csrc/common.h) reads the byte off the fp32 fields of amax: exponent field, plus one where the
    mantissa exceeds 1.75's, minus 8, floored at 0.  Restated on the bits, it is the oracle's rule for every 16-bit amax."""
    x, pats = _amax_blocks(dtype)
    want = (mx8.block_exponents(x).reshape(-1)[:len(pats)] + 127).numpy()
    bits = P.to_float(pats, dtype).numpy().view(np.uint32).astype(np.int64)
    be = (bits >> 23) + ((bits & 0x7fffff) > 0x600000)
    assert np.array_equal(np.maximum(be - 8, 0), want)


def test_tiny_bf16_amax_bytes():
    """The clamp boundary by name: amax <= 448 * 2^-127 (1120 patterns) has byte 0, up to 448 * 2^-126 byte 1, then 2."""
    x, pats = _amax_blocks(torch.bfloat16)
    b = (mx8.block_exponents(x).reshape(-1)[:len(pats)] + 127).tolist()
    assert set(b[:1120]) == {0} and set(b[1120:P.TINY_BF16_LAST]) == {1} and b[P.TINY_BF16_LAST] == 2
    assert float(P.to_float(np.array([1120], dtype=np.uint16), torch.bfloat16)[0]) == 448.0 * 2.0 ** -127


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_has_no_nan_byte_and_rounds_within_half_an_ulp(dtype):
    xs = P.every_element_sweep(dtype)
    assert 3_000_000 < xs.numel() < 6_000_000                        # one launch's worth: fp16 3.6 M, bf16 4.9 M elements
    x = xs.float()
    q, packed, ex = mx8.quantize(x)
    assert not ((q & 0x7f) == 0x7f).any(), "a finite input became an e4m3 NaN byte"
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), ex.double()).repeat_interleave(32, dim=1)
    d = q.view(torch.float8_e4m3fn).double() * scale                  # in float64: 256 * 2^120, the rounded-up top of bf16, is no fp32 number
    finite32 = d.abs() < 2.0 ** 128
    assert torch.equal(mx8.dequantize(q, ex).double()[finite32], d[finite32])
    err = (d - x.double()).abs()
    # half an ulp: 2^-10 * scale below the e4m3 normal range (spacing 2^-9), relative 2^-4 inside it (3 mantissa bits)
    bound = torch.maximum(scale * 2.0 ** -10, x.double().abs() * 2.0 ** -4)
    assert (err <= bound).all(), f"max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}"
    # round to nearest EVEN on exact ties: the stored byte is even wherever the error is exactly half a spacing
    y = (x.double() / scale).abs()
    spacing = torch.where(y < 2.0 ** -6, torch.tensor(2.0 ** -9, dtype=torch.float64), torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(y.clamp_min(2.0 ** -6))) - 3))
    tie = (err / scale == spacing / 2) & (y < 448)
    assert int(tie.sum()) > 10000 and ((q[tie] & 1) == 0).all()
    # the packed dwords are the exponents' bytes
    assert torch.equal(mx8.unpack_scales(packed, x.shape[0]), ex)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sign_of_an_underflowed_element(dtype):
    xs = P.every_element_sweep(dtype)
    x = xs.float()
    q, _, ex = mx8.quantize(x)
    scale = torch.ldexp(torch.ones((), dtype=torch.float64), ex.double()).repeat_interleave(32, dim=1)
    under = x.double().abs() <= scale * 2.0 ** -10                    # at or below the tie between zero and the smallest subnormal
    neg = torch.signbit(x)
    assert int((under & neg & (x != 0)).sum()) > 500 and int((under & ~neg & (x != 0)).sum()) > 500
    assert (q[under & neg] == 0x80).all() and (q[under & ~neg] == 0x00).all()
    assert ((q[~under] & 0x7f) != 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_contract_and_mask(dtype):
    g = torch.Generator().manual_seed(5)
    clean = torch.randn((6, 256), generator=g).to(dtype)
    x = clean.clone()
    x[1, 0], x[2, 63], x[3, 100], x[4, 255] = float("inf"), float("-inf"), float("nan"), float("inf")
    x[5, 32:64] = 0
    x[5, 40] = float("nan")
    q, packed, ex, unspec = mx8.quantize(x.float(), return_unspecified=True)
    q0, packed0, ex0 = mx8.quantize(clean.float())
    want = torch.zeros(6, 8, dtype=torch.bool)
    want[1, 0] = want[2, 1] = want[3, 3] = want[4, 7] = want[5, 1] = True
    assert torch.equal(unspec, want)
    nonfinite = ~torch.isfinite(x.float())
    assert ((q[nonfinite] & 0x7f) == 0x7f).all()
    keep = ~unspec.repeat_interleave(32, dim=1)
    keep[5, 32:64] = False                                             # this block differs between x and clean by construction
    assert torch.equal(q[keep], q0[keep])
    keep_b = ~unspec
    assert torch.equal(ex[keep_b], ex0[keep_b])
    assert len(mx8.quantize(clean.float())) == 3                       # callers that do not ask keep their three values
