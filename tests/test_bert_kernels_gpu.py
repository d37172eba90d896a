"""omg_gemm_skinny and omg_bert_embed_ln (csrc/bert.hip) on the GPU (-m gpu).  Every reference is a float64 torch-CPU computation on the
STORED operands (the values after rounding to the storage type); every bound is derived from the number formats, none is measured.

omg_gemm_skinny, per element of C with S = sum_k |a_k w_k|:
    half an ulp of the storage type at the result                      the one rounding, at the store
  + K 2^-23 S                                                           the fp32 sum of K exact products, in any order
  + 2^-22 (S + |bias| + |residual| + |result|)                          the epilogue's fp32 additions
  + 1.13 (the above, on the pre-activation) + 1e-6 + 2^-22 |gelu|       with the GELU: its slope is at most 1.13; gelu.h's form is within
                                                                        3.9e-7 of the erf form (tests/test_gelu.py)
omg_bert_embed_ln, per element, with d = 2^-23 max_i (|word_i| + |type_i| + |pos_i|) (two fp32 additions per element), sigma the row's
standard deviation, z the normalised value:
    half an ulp of the storage type at the result
  + |gamma| (1 + |z|) (2 d / sigma + (C + 8) 2^-23)                     d moves x - mean by at most 2 d and sigma by at most 2 d; the two-
                                                                        pass statistics are fp32 sums of C terms
  + 2^-22 (|gamma z| + |beta|)                                          the affine part
The rows whose three embeddings nearly cancel (|word| ~ 30, sigma ~ 0.05: the pattern of tests/test_norm_conditioning_gpu.py's offset
families) are where d / sigma is as large as the rounding itself; a sum formed in 16 bits, or in another order than (word + type) + pos
after a 16-bit rounding, misses the bound there by two orders of magnitude.

Measured on an MI355X, worst error / bound: omg_gemm_skinny 0.14 .. 0.83 in fp16 (0.97 at K = 72 and 1.00 at K = 8, where the bound is
the store's half ulp alone), 0.55 .. 1.00 in bf16; omg_bert_embed_ln 0.43 .. 0.98 in fp16, 0.85 .. 0.99 in bf16.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops

F16, BF16 = torch.float16, torch.bfloat16
MANT = {F16: 10, BF16: 7}
MIN_EXP = {F16: -14, BF16: -126}
MS = [1, 7, 16, 17, 64, 65, 130]
NKS = [(8, 8), (24, 72), (768, 768), (776, 328), (768, 3072), (3072, 768), (2304, 768)]


def _id(v):
    return str(v)[6:] if isinstance(v, torch.dtype) else None


def randn64(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def half_ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Half the spacing of `dtype` at |x| (float64), subnormals included."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** MIN_EXP[dtype]))).clamp(min=MIN_EXP[dtype])
    return 0.5 * torch.pow(2.0, e - MANT[dtype])


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


_BASE = {}


def operands(dtype, N, K):
    """A [130, K], W [N, K], bias [N], residual [130, N] in the storage type, with the float64 product and S of all 130 rows — once."""
    key = (dtype, N, K)
    if key not in _BASE:
        a = randn64(130, K, seed=N + K).to(dtype)
        w = (randn64(N, K, seed=N + K + 1) / math.sqrt(K)).to(dtype)
        bias, res = randn64(N, seed=3).to(dtype), randn64(130, N, seed=4).to(dtype)
        prod = a.double() @ w.double().T
        S = a.double().abs() @ w.double().abs().T
        _BASE[key] = (a, w, bias, res, prod, S)
    return _BASE[key]


def bound_and_ref(dtype, K, prod, S, bias, res, gelu):
    pre = prod + (bias.double()[None] if bias is not None else 0.0)
    err = K * 2.0 ** -23 * S + 2.0 ** -22 * (S + (bias.double().abs()[None] if bias is not None else 0.0) + pre.abs())
    ref = pre
    if gelu:
        ref = gelu64(pre)
        err = 1.13 * err + 1e-6 + 2.0 ** -22 * ref.abs()
    if res is not None:
        ref = ref + res.double()
        err = err + 2.0 ** -22 * (res.double().abs() + ref.abs())
    return ref, err + half_ulp(ref.abs() + err, dtype)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("N,K", NKS)
def test_gemm_skinny_against_float64(dev, dtype, N, K):
    """Every M of the list and every epilogue combination on one (N, K): a K tail (72, 328), an N tail of the 16-wide slice (3072 and 2304
    use it; 776 ends an 8-wide one), one to four active waves, all three row-block forms and a second grid row (65, 130)."""
    a, w, bias, res, prod, S = operands(dtype, N, K)
    ad, wd, bd, rd = a.to(dev), w.to(dev), bias.to(dev), res.to(dev)
    worst = 0.0
    for M in MS:
        for use_bias in (False, True):
            for gelu in (False, True):
                for use_res in (False, True):
                    out = ops.gemm_skinny(ad[:M], wd, bias=bd if use_bias else None, gelu=gelu, residual=rd[:M] if use_res else None)
                    ref, tol = bound_and_ref(dtype, K, prod[:M], S[:M], bias if use_bias else None, res[:M] if use_res else None, gelu)
                    d = (out.double().cpu() - ref).abs()
                    worst = max(worst, float((d / tol).max()))
                    assert bool((d <= tol).all()), (M, use_bias, gelu, use_res, float((d / tol).max()))
    print(f"gemm_skinny {str(dtype)[6:]} N={N} K={K}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("K", [8, 56, 64, 72, 128, 192, 256, 264, 328, 768, 3072])
def test_gemm_skinny_exact_integers(dev, dtype, K):
    """Operands in {-1, 0, 1}, an integer bias and residual: every product, every partial sum in any order and the result are exact, so the
    output is the integer answer bit for bit whatever the K split (one to four waves with a step, a tail of 8 to 56, 48 steps)."""
    g = torch.Generator().manual_seed(K)
    M, N = 37, 40
    a = torch.randint(-1, 2, (M, K), generator=g).double()
    w = torch.randint(-1, 2, (N, K), generator=g).double()
    bias, res = torch.randint(-3, 4, (N,), generator=g).double(), torch.randint(-3, 4, (M, N), generator=g).double()
    want = a @ w.T + bias[None] + res
    assert float(want.abs().max()) <= 256 and float((a.abs() @ w.abs().T).max()) < 2 ** 24, "the inputs are not exact in the storage type"
    out = ops.gemm_skinny(a.to(dtype).to(dev), w.to(dtype).to(dev), bias=bias.to(dtype).to(dev), residual=res.to(dtype).to(dev))
    assert torch.equal(out.cpu(), want.to(dtype))
    # every k position is summed exactly once: a single 1 in A at column k picks W[:, k]
    eye = torch.eye(K, dtype=dtype)
    wi = (torch.arange(N * K) % 251 - 125).reshape(N, K).to(dtype)
    assert torch.equal(ops.gemm_skinny(eye.to(dev), wi.to(dev)).cpu(), wi.T.contiguous())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("N,K", [(776, 328), (768, 3072), (3072, 768)])
@pytest.mark.parametrize("filler", ["data", 6e4, float("nan")])
def test_gemm_skinny_rows_do_not_depend_on_the_call(dev, dtype, N, K, filler):
    """Row r of the M = 130 call (first, a middle and the last row block: rows 0, 70 and 129; 70 is in the second grid row) is bitwise the
    M = 1 call on that row alone — with the other rows as drawn, filled with 6e4 (their sums overflow) and filled with NaN."""
    a, w, bias, res, _, _ = operands(dtype, N, K)
    rows = [0, 70, 129]
    big_a, big_r = a.clone(), res.clone()
    if filler != "data":
        keep = torch.zeros(130, dtype=torch.bool)
        keep[rows] = True
        big_a[~keep] = filler
        big_r[~keep] = filler
    wd, bd = w.to(dev), bias.to(dev)
    full = ops.gemm_skinny(big_a.to(dev), wd, bias=bd, gelu=True, residual=big_r.to(dev))
    for r in rows:
        one = ops.gemm_skinny(a[r:r + 1].to(dev), wd, bias=bd, gelu=True, residual=res[r:r + 1].to(dev))
        assert torch.isfinite(one).all()
        assert torch.equal(full[r:r + 1], one), r
        mid = ops.gemm_skinny(big_a[r - r % 16:r + 1].to(dev), wd, bias=bd, gelu=True, residual=big_r[r - r % 16:r + 1].to(dev))
        assert torch.equal(mid[-1:], one), ("another position in the row block", r)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
def test_gemm_skinny_strided_operands(dev, dtype):
    """Column slices of wider buffers: lda > K, ldw > K, ldr > N and a canary-filled ldc > N whose columns past N stay untouched; equal to
    the call on contiguous copies bit for bit."""
    M, N, K = 19, 776, 328
    a, w, bias, res, _, _ = operands(dtype, N, K)
    A = torch.full((M, K + 24), 7.0, dtype=dtype)
    A[:, 8:8 + K] = a[:M]
    W = torch.full((N, K + 40), -5.0, dtype=dtype)
    W[:, 16:16 + K] = w
    R = torch.full((M, N + 16), 3.0, dtype=dtype)
    R[:, 8:8 + N] = res[:M]
    Cb = torch.full((M, N + 32), 123.0, dtype=dtype, device=dev)
    Ad, Wd, Rd = A.to(dev), W.to(dev), R.to(dev)
    ops.gemm_skinny(Ad[:, 8:8 + K], Wd[:, 16:16 + K], bias=bias.to(dev), residual=Rd[:, 8:8 + N], out=Cb[:, 8:8 + N])
    want = ops.gemm_skinny(a[:M].to(dev), w.to(dev), bias=bias.to(dev), residual=res[:M].to(dev))
    assert torch.equal(Cb[:, 8:8 + N], want)
    assert bool((Cb[:, :8] == 123.0).all()) and bool((Cb[:, 8 + N:] == 123.0).all())


def test_gemm_skinny_refusals_launch_nothing(dev):
    M, N, K = 4, 16, 64
    a = torch.ones(M, K + 8, dtype=F16, device=dev)
    w = torch.ones(N, K + 8, dtype=F16, device=dev)
    c = torch.full((M, N + 8), 9.0, dtype=F16, device=dev)
    b = torch.ones(N + 8, dtype=F16, device=dev)
    lib = L.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def call(dtype=L.OMG_F16, M=M, N=N, K=K, A=a.data_ptr(), lda=K + 8, W=w.data_ptr(), ldw=K + 8, bias=None, gelu=0, res=None, ldr=0,
             Cp=c.data_ptr(), ldc=N + 8):
        rc = lib.omg_gemm_skinny(dtype, M, N, K, A, lda, W, ldw, bias, gelu, res, ldr, Cp, ldc, stream)
        return rc, (lib.omg_last_error() or b"").decode()

    assert call()[0] == 0
    torch.cuda.synchronize()
    assert bool((c[:, :N] == K).all())
    c.fill_(9.0)
    bad = [(dict(dtype=L.OMG_F32), "dtype"), (dict(A=None), "null"), (dict(W=None), "null"), (dict(Cp=None), "null"),
           (dict(M=0), ">= 1"), (dict(N=0), ">= 1"), (dict(K=0), ">= 1"), (dict(K=60), "multiples of 8"), (dict(N=12), "multiples of 8"),
           (dict(lda=K + 4), "strides"), (dict(ldw=K + 2), "strides"), (dict(ldc=N + 4), "strides"), (dict(res=c.data_ptr(), ldr=N + 1), "strides"),
           (dict(lda=K - 8), "shorter"), (dict(ldc=N - 8), "shorter"), (dict(res=c.data_ptr(), ldr=8), "shorter"),
           (dict(A=a.data_ptr() + 2), "aligned"), (dict(W=w.data_ptr() + 8), "aligned"), (dict(Cp=c.data_ptr() + 4), "aligned"),
           (dict(bias=b.data_ptr() + 2), "aligned"), (dict(gelu=2), "gelu")]
    for kw, word in bad:
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("omg_gemm_skinny") and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((c == 9.0).all()), "a refused call wrote"
    with pytest.raises(L.OmgHipError, match="omg_gemm_skinny"):
        ops.gemm_skinny(a[:, :60], w[:, :60])


# ------------------------------------------------------------------ omg_bert_embed_ln
def embed_ref(ids, types, poss, word, typ, pos, gamma, beta, eps, dtype):
    a, b, c = word.double()[ids], typ.double()[types], pos.double()[poss]
    x = a + b + c
    mean = x.mean(-1, keepdim=True)
    sigma = (x - mean).pow(2).mean(-1, keepdim=True).add(eps).sqrt()
    z = (x - mean) / sigma
    ref = z * gamma.double() + beta.double()
    Cc = x.shape[-1]
    d = 2.0 ** -23 * (a.abs() + b.abs() + c.abs()).amax(-1, keepdim=True)
    err = gamma.double().abs() * (1 + z.abs()) * (2 * d / sigma + (Cc + 8) * 2.0 ** -23) + 2.0 ** -22 * ((gamma.double() * z).abs() + beta.double().abs())
    return ref, err + half_ulp(ref.abs() + err, dtype)


def tables(dtype, Cc, n_word=37, n_type=2, n_pos=21, seed=0):
    """Word rows of magnitude ~30 (fp16) / ~8 (bf16); position row p nearly cancels word row p (mod n_pos) — their sum has a standard
    deviation of ~0.05 (fp16) / ~0.25 (bf16), a few spacings of the storage type at the rows' magnitude — the type rows are of that size."""
    big, small = (30.0, 0.05) if dtype == F16 else (8.0, 0.25)
    word = (randn64(n_word, Cc, seed=seed) * big).to(dtype)
    pos = (-word[torch.arange(n_pos) % n_word].double() + randn64(n_pos, Cc, seed=seed + 1) * small).to(dtype)
    typ = (randn64(n_type, Cc, seed=seed + 2) * small).to(dtype)
    gamma, beta = (1.0 + 0.2 * randn64(Cc, seed=seed + 3)).to(dtype), (0.1 * randn64(Cc, seed=seed + 4)).to(dtype)
    return word, typ, pos, gamma, beta


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("Cc", [8, 192, 768, 2056, 4096])
def test_bert_embed_ln_against_float64(dev, dtype, Cc):
    """Widths 8, 192, 768 (one and two vectors a lane), 2056 (five of eight, a ragged last one) and 4096 (the limit); int64 ids [2, 23]
    (rows off the four tokens a block) that cover the first and the last row of each table; half of the tokens take the position row that
    nearly cancels their word row, the others an unrelated one (a well-conditioned row)."""
    word, typ, pos, gamma, beta = tables(dtype, Cc, seed=Cc)
    n_word, n_type, n_pos = word.shape[0], typ.shape[0], pos.shape[0]
    g = torch.Generator().manual_seed(Cc)
    ids = torch.randint(0, n_word, (2, 23), generator=g)
    ids[0, 0], ids[0, 1], ids[1, -1] = 0, n_word - 1, n_pos - 1
    poss = ids % n_pos
    poss[:, 1::2] = torch.randint(0, n_pos, poss[:, 1::2].shape, generator=g)
    poss[0, 0], poss[1, -1] = 0, n_pos - 1
    types = torch.randint(0, n_type, ids.shape, generator=g)
    types[0, 0], types[0, 1] = 0, n_type - 1
    assert ids.dtype == torch.int64
    out = ops.bert_embed_ln(ids.to(dev), types.to(dev), poss.to(dev), word.to(dev), typ.to(dev), pos.to(dev), gamma.to(dev), beta.to(dev), 1e-12)
    assert out.shape == (2, 23, Cc) and out.dtype == dtype
    ref, tol = embed_ref(ids, types, poss, word, typ, pos, gamma, beta, 1e-12, dtype)
    d = (out.double().cpu() - ref).abs()
    print(f"bert_embed_ln {str(dtype)[6:]} C={Cc}: worst error / bound {float((d / tol).max()):.3f}")
    assert bool((d <= tol).all()), float((d / tol).max())
    # the cancelling rows are what the bound is about: the same sum formed in the storage type misses it
    x16 = ((word[ids] + typ[types]) + pos[poss]).double()
    z16 = (x16 - x16.mean(-1, keepdim=True)) / (x16 - x16.mean(-1, keepdim=True)).pow(2).mean(-1, keepdim=True).add(1e-12).sqrt()
    assert not bool((((z16 * gamma.double() + beta.double()) - ref).abs() <= tol).all()), "the inputs do not tell a 16-bit sum from an fp32 one"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
def test_bert_embed_ln_clamps_ids_into_their_tables(dev, dtype):
    """Ids below 0 and at or above the table size give what the clamped ids give, bit for bit: the clamp is in the address computation."""
    word, typ, pos, gamma, beta = tables(dtype, 192, seed=5)
    n_word, n_type, n_pos = word.shape[0], typ.shape[0], pos.shape[0]
    ids = torch.tensor([[-1, -(2 ** 62), n_word, n_word + 1000, 2 ** 40, 3, 0, n_word - 1]])
    types = torch.tensor([[0, n_type, -7, 2 ** 33, 1, -1, n_type + 5, 0]])
    poss = torch.tensor([[n_pos, 2, -3, n_pos - 1, -(2 ** 50), 2 ** 31, 0, n_pos + 1]])
    args = [t.to(dev) for t in (word, typ, pos, gamma, beta)]
    got = ops.bert_embed_ln(ids.to(dev), types.to(dev), poss.to(dev), *args, 1e-12)
    want = ops.bert_embed_ln(ids.clamp(0, n_word - 1).to(dev), types.clamp(0, n_type - 1).to(dev), poss.clamp(0, n_pos - 1).to(dev), *args, 1e-12)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want)


def test_bert_embed_ln_refusals(dev):
    word, typ, pos, gamma, beta = (t.to(dev) for t in tables(F16, 16))
    ids = torch.zeros(1, 4, dtype=torch.int64, device=dev)
    with pytest.raises(L.OmgHipError, match="int64"):
        ops.bert_embed_ln(ids.int(), ids, ids, word, typ, pos, gamma, beta, 1e-12)
    wide = torch.zeros(2, 4104, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError, match="at most 4096"):
        ops.bert_embed_ln(ids, ids, ids, wide, wide, wide, wide[0], wide[0], 1e-12)
    lib = L.lib()
    y = torch.zeros(4, 16, dtype=F16, device=dev)
    rc = lib.omg_bert_embed_ln(L.OMG_F16, 4, 12, ids.data_ptr(), ids.data_ptr(), ids.data_ptr(), word.data_ptr(), 4, typ.data_ptr(), 2,
                               pos.data_ptr(), 4, gamma.data_ptr(), beta.data_ptr(), 1e-12, y.data_ptr(), 16, None)
    assert rc != 0 and b"multiple of 8" in lib.omg_last_error()
    rc = lib.omg_bert_embed_ln(L.OMG_F16, 4, 16, ids.data_ptr(), None, ids.data_ptr(), word.data_ptr(), 4, typ.data_ptr(), 2,
                               pos.data_ptr(), 4, gamma.data_ptr(), beta.data_ptr(), 1e-12, y.data_ptr(), 16, None)
    assert rc != 0 and b"null" in lib.omg_last_error()
