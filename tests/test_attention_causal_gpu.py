"""`omg_attn_fwd_causal` (csrc/attn_v6.h, the causal instance of the resident-K/V kernel) on the GPU (-m gpu).

Mask rule: key j is visible to query i iff j <= i and j < Nkv (top-left alignment).  Reference: a float64 masked softmax on the
16-bit-rounded inputs (CPU).  Tolerance: the project's kernel-level one — rtol 2e-3 / atol 2e-3 in fp16, 1.6e-2 in bf16.
B = 2, heads = 2 (head and batch strides matter), N(0, 1) inputs, scale 1/8.

1. Parity at every edge of the kernel: Nq = Nkv around every 16-key block, the 32-row wave step and the 64-key tile; more rows than
   one 128-row step, rows past the last key, more keys than rows.
2. Exact answers, which catch a leak of any size: row 0 is V[0]; Q = 0 with V = 1 gives 1; rows <= i0 keep their bits when every key
   after i0 is overwritten with +-6e4; a masked score 200 above the visible ones (the lazy reference maximum must not see it).
3. accumulate with out_scale, borrowed Q / K (qk_src), O as a strided view inside a canary-filled buffer.
4. Host-side rejections: more than 128 keys; row-major V without a V^T image."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
TOL = {F16: dict(rtol=2e-3, atol=2e-3), BF16: dict(rtol=1.6e-2, atol=1.6e-2)}
B, HEADS, SCALE = 2, 2, 0.125
C_ = HEADS * 64

SQUARE = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 77, 80, 127, 128]
RECT = [(130, 128), (130, 77), (40, 100)]


def inputs(nq, nkv, dtype, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + nq * 131 + nkv)
    return tuple(torch.randn(B, n, C_, generator=g).to(dtype) for n in (nq, nkv, nkv))


def reference(q, k, v, scale=SCALE):
    """float64 softmax over the visible keys, on the stored 16-bit values: (B, Nq, heads * 64)."""
    nq, nkv = q.shape[1], k.shape[1]
    qh, kh, vh = (t.double().cpu().view(B, -1, HEADS, 64).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    hidden = torch.arange(nkv)[None, :] > torch.arange(nq)[:, None]
    s = s.masked_fill(hidden, float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).transpose(1, 2).reshape(B, nq, C_)


def run(q, k, v, dev, **kw):
    q, k, v = q.to(dev), k.to(dev), v.to(dev)
    vt = ops.transpose_v(v, HEADS)
    return ops.attention(q, k, vt, HEADS, SCALE, causal=True, **kw)


def close(got, ref, dtype):
    got = got.double().cpu()
    err = (got - ref).abs()
    print(f"max |d| {err.max().item():.3e} at |ref| <= {ref.abs().max().item():.2f}")
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, ref, **TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq,nkv", [(n, n) for n in SQUARE] + RECT)
def test_parity_at_every_edge(dev, dtype, nq, nkv):
    q, k, v = inputs(nq, nkv, dtype)
    close(run(q, k, v, dev), reference(q, k, v), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_0_is_the_first_value_row(dev, dtype):
    q, k, v = inputs(80, 80, dtype, seed=1)
    out = run(q, k, v, dev)
    assert torch.equal(out[:, 0].cpu(), v[:, 0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [80, 128])
def test_zero_queries_average_a_constant_value_exactly(dev, dtype, n):
    q, k, v = inputs(n, n, dtype, seed=2)
    out = run(torch.zeros_like(q), k, torch.ones_like(v), dev)
    assert torch.equal(out.cpu(), torch.ones_like(v))


@pytest.fixture(scope="module")
def unperturbed(dev):
    res = {}
    for dtype in DTYPES:
        q, k, v = inputs(80, 80, dtype, seed=3)
        res[dtype] = (q, k, v, run(q, k, v, dev).cpu())
    return res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i0", [0, 15, 16, 63, 64, 76])
def test_rows_do_not_depend_on_later_keys(dev, unperturbed, dtype, i0):
    q, k, v, base = unperturbed[dtype]
    sign = torch.where((torch.arange(79 - i0)[:, None] + torch.arange(C_)[None, :]) % 3 == 0, -1.0, 1.0)      # (keys after i0, C): mixed signs
    k2, v2 = k.clone(), v.clone()
    k2[:, i0 + 1:] = (6e4 * sign).to(dtype)
    v2[:, i0 + 1:] = (-6e4 * sign).to(dtype)
    out = run(q, k2, v2, dev).cpu()
    assert torch.equal(out[:, : i0 + 1], base[:, : i0 + 1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("first_high", [3, 40, 70])
def test_a_masked_score_far_above_the_visible_ones_does_not_move_the_reference_maximum(dev, dtype, first_high):
    """Channel 0 of every head: q = 16, k = 100 from key `first_high` on and 0 below: those keys score 0.125 * 1600 = 200 above the
    rest.  Rows below `first_high` have them masked — in the first tile (3, 40) and in the second (70: rows 64 .. 69) — and a
    maximum taken before the mask would leave them 2^-288 of weight: 0 / 0."""
    q, k, v = inputs(80, 80, dtype, seed=4)
    q, k = q.clone(), k.clone()
    q[:, :, 0::64] = 16.0
    k[:, :, 0::64] = 0.0
    k[:, first_high:, 0::64] = 100.0
    close(run(q, k, v, dev), reference(q, k, v), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulate_with_out_scale(dev, dtype):
    q, k, v = inputs(77, 77, dtype, seed=5)
    old = torch.randn(B, 77, C_, generator=torch.Generator().manual_seed(6)).to(dtype)
    out = old.to(dev)
    run(q, k, v, dev, out=out, accumulate=True, out_scale=0.5)
    close(out, old.double() + 0.5 * reference(q, k, v), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_borrowed_queries_and_keys(dev, dtype):
    q, k, v = inputs(77, 77, dtype, seed=7)
    src = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    close(run(q, k, v, dev, qk_src=src), reference(q[[1, 0]], k[[1, 0]], v), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_output_leaves_every_other_element_alone(dev, dtype):
    nq = 77
    q, k, v = inputs(nq, nq, dtype, seed=8)
    dense = run(q, k, v, dev)
    canary = 123.0
    buf = torch.full((B, nq + 5, C_ + 24), canary, dtype=dtype, device=dev)
    view = buf[:, :nq, 8:8 + C_]                       # row stride C + 24, a gap of rows between samples, 16 bytes into the row
    run(q, k, v, dev, out=view)
    assert torch.equal(view, dense)
    owned = torch.zeros_like(buf, dtype=torch.bool)
    owned[:, :nq, 8:8 + C_] = True
    assert bool((buf[~owned] == canary).all())


def test_more_than_128_keys_are_rejected_with_the_limit_in_the_message(dev):
    q, k, v = inputs(129, 129, F16, seed=9)
    with pytest.raises(L.OmgHipError, match="128"):
        run(q, k, v, dev)


def test_row_major_v_without_its_transposed_image_is_rejected(dev):
    q, k, v = (t.to(dev) for t in inputs(80, 80, F16, seed=9))
    out = torch.empty_like(q)
    a = ops._attn_args(q, k, None, HEADS, 80, SCALE, None, out, False, 1.0)
    a.V, a.ldv, a.v_bstride = v.data_ptr(), v.stride(1), v.stride(0)
    assert L.lib().omg_attn_fwd_causal(C.byref(a), None) == -1
    assert b"Vt" in L.lib().omg_last_error()
