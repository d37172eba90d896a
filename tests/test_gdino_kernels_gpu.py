"""omg_msdeform_attn, omg_attn_bi_vision, omg_attn_bi_text and omg_attn_masked (csrc/gdino.hip) against float64 compositions of the
same 16-bit operands (-m gpu).

Deformable attention.  The reference is the library's composition in float64: softmax of the logits, loc = ref + off / (W, H),
grid = 2 loc - 1, F.grid_sample(bilinear, zeros, align_corners=False) per level on the (masked) value, the weighted sum.  The bound per
element is one rounding of the storage type on the float64 result r plus what fp32 arithmetic may add before that rounding:

    |out - r| <= u16 |r| + E32 (1 + u16) + tiny,        u16 = 2^-11 (fp16) | 2^-8 (bf16),   tiny = 2^-25 (fp16 subnormal spacing / 2)
    E32 = 2^-24 vmax (K_SOFTMAX + K_SUM + K_COORD),      vmax = max |value|

  K_SUM     = 64: the 64 fused multiply-adds of the taps in sequence, |sum| <= vmax (the weights sum to at most 1).
  K_SOFTMAX = 5 A + 24, A = log2(e) max |logit|: the exponent's argument logit log2 e - max is two roundings of values up to 2 A and a
              constant rounded to fp32 (<= 2.5 A units, times ln 2 < 1 on the exponential), exp2 of the hardware 1 ulp = 2 units; that
              twice (numerator and sum), 15 additions, the division, the product with it, and three roundings in (1 - lx)(1 - ly) a.
  K_COORD   = 4 (3 Dmax + 5), Dmax = the largest level side: the pixel coordinate fma(ref, W, off - 0.5) carries two roundings of
              values up to 2 W + 2.5 and W + 2 (locations further out sample nothing on either side); the sampled value is continuous
              and piecewise bilinear in the coordinate with slope at most 2 vmax (zero padding included), for x and for y.

The measured maximum of |out - r| / bound is printed beside the bound.

Attention (bi-attention at head_dim 256, masked attention at head_dim 64).  The rule of tests/test_attention_conditioning_gpu.py with
its constants C_MAX = C_RMS = 4 and its floors, `truth` from tests/_attn_model.py on masked scores.  tests/_attn_model.py::model does
not apply as it stands: it rounds a PRE-SCALED query Q' = round16(q scale log2 e) to 16 bits, which these kernels do not do (they scale
the fp32 score in the exponent), and it knows no mask.  `model_masked` below keeps the model's other rounding points and nothing else:
exact scores on the 16-bit operands, P = round16(exp2(S - rowmax)), O = P v / sum(P) with the sum on the rounded P.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from tests import _attn_model as M

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
C_MAX = 4.0
C_RMS = 4.0
LOG2E = 1.4426950408889634


def _id(v):
    if isinstance(v, torch.dtype):
        return "fp16" if v == F16 else "bf16"
    if isinstance(v, (tuple, list)):
        return "-".join(_id(i) or str(i) for i in v)
    return None


def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ multi-scale deformable attention
LEVELS4 = [(13, 19), (7, 10), (4, 5), (2, 3)]
HEADS = 8


def starts_of(shapes):
    out, s = [], 0
    for h, w in shapes:
        out.append(s)
        s += h * w
    return out, s


def msd_case(dtype, B, shapes, Nq, seed, with_mask):
    """value N(0, 1); logits N(0, 2.5^2) (far from uniform); offsets N(0, 3^2) pixels; refs uniform in [0, 1].  Queries 0 .. 5 of every
    sample are the special locations: far outside on both sides, on the border (loc = 0 and loc = 1), exactly on pixel centres."""
    Lv = len(shapes)
    _, N = starts_of(shapes)
    value = randn(B, N, HEADS * 32, seed=seed)
    off = randn(B, Nq, HEADS, Lv, 4, 2, seed=seed + 1, scale=3.0)
    lg = randn(B, Nq, HEADS, Lv * 4, seed=seed + 2, scale=2.5)
    ref = rand(B, Nq, Lv, 2, seed=seed + 3)
    n = min(Nq, 6)
    for q in range(n):
        kind = q % 6
        if kind == 0:
            off[:, q] = 1000.0
        elif kind == 1:
            off[:, q] = -1000.0
        elif kind == 2:
            off[:, q], ref[:, q] = 0.0, 0.0
        elif kind == 3:
            off[:, q], ref[:, q] = 0.0, 1.0
        else:                                   # pixel centres: ref = 0, off = integer + 0.5 -> pixel coordinate = the integer, exactly
            ref[:, q] = 0.0
            off[:, q] = torch.floor(rand(B, HEADS, Lv, 4, 2, seed=seed + 4 + q) * 4.0) + 0.5
    ow = torch.cat([off.reshape(B, Nq, -1), lg.reshape(B, Nq, -1)], dim=-1).to(dtype)
    mask = None
    if with_mask:
        mask = rand(B, N, seed=seed + 9) > 0.3
    return value.to(dtype), ow, ref, mask


def msd_truth(value, ow, ref, shapes, mask):
    """float64, as GroundingDinoMultiscaleDeformableAttention composes it (multi_scale_deformable_attention): [B, Nq, heads 32]."""
    B, N, _ = value.shape
    Nq, Lv = ow.shape[1], len(shapes)
    v = value.double()
    if mask is not None:
        v = v.masked_fill(~mask[..., None], 0.0)
    v = v.view(B, N, HEADS, 32)
    ow = ow.double()
    off = ow[..., :HEADS * Lv * 8].view(B, Nq, HEADS, Lv, 4, 2)
    a = torch.softmax(ow[..., HEADS * Lv * 8:].view(B, Nq, HEADS, Lv * 4), dim=-1).view(B, Nq, HEADS, Lv, 4)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    loc = ref.double()[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    grids = 2.0 * loc - 1.0
    starts, _ = starts_of(shapes)
    out = torch.zeros(B * HEADS, 32, Nq, dtype=torch.float64)
    for l, (h, w) in enumerate(shapes):
        vl = v[:, starts[l]:starts[l] + h * w].permute(0, 2, 3, 1).reshape(B * HEADS, 32, h, w)
        gl = grids[:, :, :, l].transpose(1, 2).reshape(B * HEADS, Nq, 4, 2)
        s = F.grid_sample(vl, gl, mode="bilinear", padding_mode="zeros", align_corners=False)          # [B heads, 32, Nq, 4]
        al = a[:, :, :, l].transpose(1, 2).reshape(B * HEADS, 1, Nq, 4)
        out += (s * al).sum(-1)
    return out.view(B, HEADS, 32, Nq).permute(0, 3, 1, 2).reshape(B, Nq, HEADS * 32)


def msd_bound(dtype, truth, value, ow, shapes):
    Lv = len(shapes)
    u16 = 2.0 ** -11 if dtype == F16 else 2.0 ** -8
    vmax = float(value.double().abs().max())
    A = LOG2E * float(ow[..., HEADS * Lv * 8:].double().abs().max())
    dmax = max(max(s) for s in shapes)
    k = (5.0 * A + 24.0) + 64.0 + 4.0 * (3.0 * dmax + 5.0)
    e32 = 2.0 ** -24 * vmax * k
    return u16 * truth.abs() + e32 * (1.0 + u16) + 2.0 ** -25, k


def run_msd(dev, value, ow, ref, shapes, mask, **kw):
    return ops.msdeform_attn(value.to(dev), ow.to(dev), ref.to(dev), shapes, heads=HEADS, mask=None if mask is None else mask.to(dev), **kw)


MSD_SHAPES = [LEVELS4, [(1, 1)], [(1, 7)], [(5, 1)], [(13, 19)]]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shapes", MSD_SHAPES, ids=_id)
def test_msdeform_against_float64(dev, shapes, B, with_mask, dtype):
    _, N = starts_of(shapes)
    Nq = N if len(shapes) == 4 else 37
    value, ow, ref, mask = msd_case(dtype, B, shapes, Nq, seed=N * 7 + B, with_mask=with_mask)
    out = run_msd(dev, value, ow, ref, shapes, mask)
    truth = msd_truth(value, ow, ref, shapes, mask)
    bound, k = msd_bound(dtype, truth, value, ow, shapes)
    err = (out.double().cpu() - truth).abs()
    ratio = float((err / bound).max())
    print(f"msdeform {_id(dtype)} {_id(shapes)} B{B} mask{int(with_mask)}: K = {k:.0f}, max err {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    assert bool(torch.isfinite(out).all())
    assert float(truth.abs().max()) > 0.1
    assert ratio <= 1.0, f"max |out - truth| / bound = {ratio:.3f}"


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_msdeform_dominant_logit_on_a_pixel_centre_is_the_value_row(dev, dtype):
    """One logit 200 above the others (their exponentials are zero in fp32) and its location on a pixel centre (ref = 0, off = integer
    + 0.5: the pixel coordinate is the integer exactly): weight 1 on one corner of one tap -> the value row, bit for bit."""
    shapes = LEVELS4
    starts, N = starts_of(shapes)
    B, Nq, Lv = 2, 40, 4
    value, ow, ref, _ = msd_case(dtype, B, shapes, Nq, seed=21, with_mask=False)
    off = ow[..., :HEADS * Lv * 8].float().view(B, Nq, HEADS, Lv, 4, 2).clone()
    lg = torch.full((B, Nq, HEADS, Lv * 4), -200.0)
    g = torch.Generator().manual_seed(5)
    want = torch.empty(B, Nq, HEADS, 32, dtype=dtype)
    ref = torch.zeros(B, Nq, Lv, 2)
    for b in range(B):
        for q in range(Nq):
            for h in range(HEADS):
                l = int(torch.randint(0, Lv, (1,), generator=g))
                pt = int(torch.randint(0, 4, (1,), generator=g))
                Hl, Wl = shapes[l]
                iy, ix = int(torch.randint(0, Hl, (1,), generator=g)), int(torch.randint(0, Wl, (1,), generator=g))
                lg[b, q, h, l * 4 + pt] = 0.0
                off[b, q, h, l, pt, 0], off[b, q, h, l, pt, 1] = ix + 0.5, iy + 0.5
                want[b, q, h] = value[b, starts[l] + iy * Wl + ix, h * 32:(h + 1) * 32]
    ow = torch.cat([off.reshape(B, Nq, -1), lg.reshape(B, Nq, -1)], dim=-1).to(dtype)
    out = run_msd(dev, value, ow, ref, shapes, None).cpu()
    assert torch.equal(out.view(torch.int16), want.reshape(B, Nq, -1).view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_msdeform_masked_rows_read_as_zeros(dev, dtype):
    """Every value row masked: zeros, bit for bit (not a NaN from a division, not a sampled value)."""
    shapes = LEVELS4
    _, N = starts_of(shapes)
    value, ow, ref, _ = msd_case(dtype, 2, shapes, 50, seed=22, with_mask=False)
    out = run_msd(dev, value, ow, ref, shapes, torch.zeros(2, N, dtype=torch.bool)).cpu()
    assert bool((out.view(torch.int16) == 0).all())
    # and a mask of ones is no mask
    a = run_msd(dev, value, ow, ref, shapes, torch.ones(2, N, dtype=torch.bool))
    b = run_msd(dev, value, ow, ref, shapes, None)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_msdeform_strided_operands_and_canaries(dev, dtype):
    shapes = LEVELS4
    _, N = starts_of(shapes)
    B, Nq = 2, 70
    value, ow, ref, mask = msd_case(dtype, B, shapes, Nq, seed=23, with_mask=True)
    dense = run_msd(dev, value, ow, ref, shapes, mask)
    buf = torch.full((B * Nq + 3, 256 + 8), -7.25, dtype=dtype, device=dev)
    got = run_msd(dev, value, ow, ref, shapes, mask, out=buf[:B * Nq].view(B, Nq, 264))
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:B * Nq, :256].reshape(B, Nq, 256).view(torch.int16), dense.view(torch.int16))
    assert bool((buf[:B * Nq, 256:] == -7.25).all()) and bool((buf[B * Nq:] == -7.25).all())
    wide_v = torch.zeros(B, N, 256 + 16, dtype=dtype, device=dev)
    wide_v[..., :256] = value.to(dev)
    wide_ow = torch.zeros(B, Nq, 384 + 8, dtype=dtype, device=dev)
    wide_ow[..., :384] = ow.to(dev)
    again = ops.msdeform_attn(wide_v[..., :256], wide_ow[..., :384], ref.to(dev), shapes, heads=HEADS, mask=mask.to(dev))
    assert torch.equal(again.view(torch.int16), dense.view(torch.int16))


def test_msdeform_batched_equals_single(dev):
    shapes = LEVELS4
    _, N = starts_of(shapes)
    value, ow, ref, mask = msd_case(F16, 2, shapes, N, seed=24, with_mask=True)
    both = run_msd(dev, value, ow, ref, shapes, mask)
    one = run_msd(dev, value[1:], ow[1:], ref[1:], shapes, mask[1:])
    assert torch.equal(both[1:], one)


def test_msdeform_rejects_what_it_cannot_run(dev):
    shapes = LEVELS4
    _, N = starts_of(shapes)
    value, ow, ref, _ = msd_case(F16, 1, shapes, 8, seed=25, with_mask=False)
    out = torch.full((1, 8, 256), -7.25, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError, match="head_dim 32"):
        ops.msdeform_attn(value.to(dev), ow.to(dev)[..., :192], ref.to(dev), shapes, heads=4, out=out)           # 4 heads of 64
    with pytest.raises(L.OmgHipError, match="beyond N"):
        ops.msdeform_attn(value.to(dev), ow.to(dev), ref.to(dev), shapes, heads=HEADS, level_start=[0, 247, 317, 338], out=out)
    with pytest.raises(L.OmgHipError, match="levels"):
        ops.msdeform_attn(value.to(dev), ow.to(dev), ref.to(dev), shapes + [(1, 1)], heads=HEADS, out=out)
    ow3 = torch.zeros(1, 8, HEADS * 4 * 3 * 3, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError, match="points 4"):
        ops.msdeform_attn(value.to(dev), ow3, ref.to(dev), shapes, heads=HEADS, points=3, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()), "a refused call launched something"


# ------------------------------------------------------------------ attention: the rule and its references
def masked_scores(q, k, scale, keep):
    """float64 scores in natural units, excluded keys at -inf; keep broadcasts against [..., Nq, Nk] or is None."""
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    if keep is not None:
        s = s.masked_fill(~keep, float("-inf"))
    return s


def truth_masked(q, k, v, scale, keep):
    return torch.softmax(masked_scores(q, k, scale, keep), dim=-1) @ v.double()


def model_masked(q, k, v, scale, keep):
    s = masked_scores(q, k, scale, keep) * LOG2E
    p = M.round16(torch.exp2(s - s.amax(dim=-1, keepdim=True)), q.dtype)
    return M.round16((p @ v.double()) / p.sum(dim=-1, keepdim=True), q.dtype)


def bounded(tag, dtype, out, truth, model_rounded):
    e_k = (out.double().cpu() - truth).abs()
    e_m = (model_rounded - truth).abs()
    floor = M.ulp(dtype) * float(truth.abs().max())
    floor_rms = floor / math.sqrt(12.0)
    mk, mm, rk, rm = float(e_k.max()), float(e_m.max()), M.rms(e_k), M.rms(e_m)
    print(f"{tag}: max e_k {mk:.3e} e_m {mm:.3e} floor {floor:.3e}; rms e_k {rk:.3e} e_m {rm:.3e}")
    assert bool(torch.isfinite(out).all()), f"{tag}: non-finite output"
    assert mk <= max(floor, C_MAX * mm), f"{tag}: max error {mk:.3e} > max({floor:.3e}, {C_MAX} * {mm:.3e})"
    assert rk <= max(floor_rms, C_RMS * rm), f"{tag}: rms error {rk:.3e} > max({floor_rms:.3e}, {C_RMS} * {rm:.3e})"


def heads_of(t, heads, d):
    """(B, N, heads d) -> (B, heads, N, d)"""
    return t.reshape(t.shape[0], t.shape[1], heads, d).permute(0, 2, 1, 3)


def merged(t):
    """(B, heads, N, d) -> (B, N, heads d)"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)


# ------------------------------------------------------------------ bi-attention, head_dim 256
BH, BD = 4, 256
BSCALE = BD ** -0.5
CHUNK = 64          # omg_attn_bi_text_chunk(N) for N <= 4096 (asserted below)


def bi_case(dtype, B, N, T, seed):
    """q and k at 1.7: scale q.k has a standard deviation near 3, the softmax rows are far from uniform."""
    vis = randn(B, N, 2 * BH * BD, seed=seed)
    txt = randn(B, T, 2 * BH * BD, seed=seed + 1)
    vis[..., :BH * BD] *= 1.7
    txt[..., :BH * BD] *= 1.7
    return vis.to(dtype), txt.to(dtype)


def bi_masks(kind, B, N, T, seed):
    """(text keep [B, T], vision keep [B, N]) or None: `partial` drops about a third of either side (never everything); `chunk` drops
    the whole second chunk of image keys as well (or the first, where there is one chunk only and more keys behind... there are none:
    then the first half)."""
    if kind == "none":
        return None, None
    tk = rand(B, T, seed=seed + 5) > 0.35
    vk = rand(B, N, seed=seed + 6) > 0.35
    tk[:, 0] = True
    vk[:, N - 1] = True
    if kind == "chunk":
        if N > CHUNK:
            vk[:, CHUNK:min(N - 1, 2 * CHUNK)] = False
        else:
            vk[:, :N // 2] = False
    return tk, vk


def bi_split(vis, txt):
    hd = BH * BD
    q, vv = heads_of(vis[..., :hd], BH, BD), heads_of(vis[..., hd:], BH, BD)
    k, tv = heads_of(txt[..., :hd], BH, BD), heads_of(txt[..., hd:], BH, BD)
    return q, vv, k, tv


BI_NT = ([(n, 11) for n in (1, 63, 64, 65, 343, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)]
         + [(343, t) for t in (1, 64, 65, 256)] + [(65, 256), (1, 1)])
BI_NT = sorted(set(BI_NT))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("masks", ["none", "partial", "chunk"])
@pytest.mark.parametrize("NT", BI_NT, ids=_id)
def test_bi_attention_against_float64(dev, NT, masks, B, dtype):
    N, T = NT
    assert ops.attn_bi_text_chunk(N) == CHUNK
    vis, txt = bi_case(dtype, B, N, T, seed=N * 3 + T)
    tk, vk = bi_masks(masks, B, N, T, seed=N + T)
    q, vv, k, tv = bi_split(vis, txt)
    ov = ops.attn_bi_vision(vis.to(dev), txt.to(dev), BH, BSCALE, text_mask=None if tk is None else tk.to(dev))
    ot = ops.attn_bi_text(vis.to(dev), txt.to(dev), BH, BSCALE, vision_mask=None if vk is None else vk.to(dev))
    keep_t = None if tk is None else tk[:, None, None, :]
    keep_v = None if vk is None else vk[:, None, None, :]
    tag = f"{_id(dtype)} N{N} T{T} {masks} B{B}"
    bounded("bi-vision " + tag, dtype, ov, merged(truth_masked(q, k, tv, BSCALE, keep_t)), merged(model_masked(q, k, tv, BSCALE, keep_t)))
    bounded("bi-text " + tag, dtype, ot, merged(truth_masked(k, q, vv, BSCALE, keep_v)), merged(model_masked(k, q, vv, BSCALE, keep_v)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bi_text_chunks_of_several_tiles(dev, dtype):
    """N beyond 4096: a chunk is two 64-key tiles (the online softmax inside a workgroup), the last chunk a few keys, and a mask that
    empties whole chunks."""
    N, T, B = 4100, 11, 1
    chunk = ops.attn_bi_text_chunk(N)
    assert chunk == 128 and ops.attn_bi_text_chunk(19947) == 320 and ops.attn_bi_text_chunk(4096) == 64
    vis, txt = bi_case(dtype, B, N, T, seed=77)
    vk = rand(B, N, seed=78) > 0.35
    vk[:, chunk:3 * chunk] = False
    vk[:, 5 * chunk:5 * chunk + 64] = False
    q, vv, k, _ = bi_split(vis, txt)
    ot = ops.attn_bi_text(vis.to(dev), txt.to(dev), BH, BSCALE, vision_mask=vk.to(dev))
    keep = vk[:, None, None, :]
    bounded(f"bi-text {_id(dtype)} N{N}", dtype, ot, merged(truth_masked(k, q, vv, BSCALE, keep)), merged(model_masked(k, q, vv, BSCALE, keep)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("NT", [(129, 11), (343, 65), (65, 256)], ids=_id)
def test_bi_equal_scores_give_the_mean_of_v(dev, NT, dtype):
    """q = 0: every probability is equal; v on the grid of eighths, so the sums are exact and the result is one rounding of the mean
    over the keys that take part."""
    N, T = NT
    B, hd = 2, BH * BD
    vis, txt = bi_case(dtype, B, N, T, seed=31)
    vis[..., :hd] = 0
    vis[..., hd:] = (torch.round(randn(B, N, hd, seed=32) * 8.0) / 8.0).to(dtype)
    txt[..., hd:] = (torch.round(randn(B, T, hd, seed=33) * 8.0) / 8.0).to(dtype)
    tk, vk = bi_masks("chunk", B, N, T, seed=34)
    ov = ops.attn_bi_vision(vis.to(dev), txt.to(dev), BH, BSCALE, text_mask=tk.to(dev)).double().cpu()
    ot = ops.attn_bi_text(vis.to(dev), txt.to(dev), BH, BSCALE, vision_mask=vk.to(dev)).double().cpu()
    for b in range(B):
        want_v = txt[b, tk[b], hd:].double().mean(0)
        want_t = vis[b, vk[b], hd:].double().mean(0)
        assert float((ov[b] - want_v).abs().max()) <= M.ulp(dtype) * float(want_v.abs().max())
        assert float((ot[b] - want_t).abs().max()) <= M.ulp(dtype) * float(want_t.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("NT", [(129, 11), (343, 65)], ids=_id)
def test_bi_dominant_key_gives_its_value_row(dev, NT, dtype):
    """Row r's query is 8 x the key j(r): its score is hundreds above every other one, the other probabilities round to zero (and a
    chunk without the key folds in with weight 2^-400 = 0): the output is the key's value row, bit for bit."""
    N, T = NT
    B, hd = 1, BH * BD
    vis, txt = bi_case(dtype, B, N, T, seed=41)
    g = torch.Generator().manual_seed(42)
    # vision side: image row n looks at text key jt[n]
    jt = torch.randint(0, T, (N,), generator=g)
    vis_q = vis.clone()
    vis_q[0, :, :hd] = (txt[0, jt, :hd].float() * 8.0).to(dtype)
    ov = ops.attn_bi_vision(vis_q.to(dev), txt.to(dev), BH, BSCALE).cpu()
    assert torch.equal(ov[0].view(torch.int16), txt[0, jt, hd:].contiguous().view(torch.int16))
    # text side: text token t looks at image key jn[t]
    jn = torch.randint(0, N, (T,), generator=g)
    txt_k = txt.clone()
    txt_k[0, :, :hd] = (vis[0, jn, :hd].float() * 8.0).to(dtype)
    ot = ops.attn_bi_text(vis.to(dev), txt_k.to(dev), BH, BSCALE).cpu()
    assert torch.equal(ot[0].view(torch.int16), vis[0, jn, hd:].contiguous().view(torch.int16))


def test_bi_batched_equals_single_and_strides(dev):
    N, T, B = 343, 37, 2
    vis, txt = bi_case(F16, B, N, T, seed=51)
    tk, vk = bi_masks("partial", B, N, T, seed=52)
    v_d, t_d, tk_d, vk_d = vis.to(dev), txt.to(dev), tk.to(dev), vk.to(dev)
    ov = ops.attn_bi_vision(v_d, t_d, BH, BSCALE, text_mask=tk_d)
    ot = ops.attn_bi_text(v_d, t_d, BH, BSCALE, vision_mask=vk_d)
    assert torch.equal(ov[1:], ops.attn_bi_vision(v_d[1:], t_d[1:], BH, BSCALE, text_mask=tk_d[1:]))
    assert torch.equal(ot[1:], ops.attn_bi_text(v_d[1:], t_d[1:], BH, BSCALE, vision_mask=vk_d[1:]))
    # padded rows, padded samples and a canary-filled output
    wv = torch.zeros(B, N + 2, 2048 + 8, dtype=F16, device=dev)
    wv[:, :N, :2048] = v_d
    wt = torch.zeros(B, T + 1, 2048 + 16, dtype=F16, device=dev)
    wt[:, :T, :2048] = t_d
    buf = torch.full((B, N + 1, 1024 + 8), -7.25, dtype=F16, device=dev)
    ops.attn_bi_vision(wv[:, :N, :2048], wt[:, :T, :2048], BH, BSCALE, text_mask=tk_d, out=buf[:, :N, :1024])
    assert torch.equal(buf[:, :N, :1024], ov) and bool((buf[:, N:] == -7.25).all()) and bool((buf[:, :, 1024:] == -7.25).all())
    buf = torch.full((B, T + 1, 1024 + 8), -7.25, dtype=F16, device=dev)
    ops.attn_bi_text(wv[:, :N, :2048], wt[:, :T, :2048], BH, BSCALE, vision_mask=vk_d, out=buf[:, :T, :1024])
    assert torch.equal(buf[:, :T, :1024], ot) and bool((buf[:, T:] == -7.25).all()) and bool((buf[:, :, 1024:] == -7.25).all())


def test_bi_rejects_what_it_cannot_run(dev):
    vis, txt = bi_case(F16, 1, 8, 257, seed=61)
    out = torch.full((1, 8, 1024), -7.25, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError, match="T at most 256"):
        ops.attn_bi_vision(vis.to(dev), txt.to(dev), BH, BSCALE, out=out)
    out_t = torch.full((1, 257, 1024), -7.25, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError, match="T at most 256"):
        ops.attn_bi_text(vis.to(dev), txt.to(dev), BH, BSCALE, out=out_t)
    v_d, t_d = vis.to(dev), txt[:, :16].to(dev)
    rc = L.lib().omg_attn_bi_vision(L.OMG_F16, 1, BH, 8, 16, v_d.data_ptr() + 2, 2048, 8 * 2048, t_d.data_ptr(), 2048, 16 * 2048, None,
                                    BSCALE, out.data_ptr(), 1024, 8 * 1024, 0)
    assert rc == -1 and b"aligned" in L.lib().omg_last_error()
    rc = L.lib().omg_attn_bi_text(L.OMG_F16, 1, BH, 8, 16, v_d.data_ptr(), 2048, 8 * 2048, t_d.data_ptr(), 2048, 16 * 2048, None,
                                  BSCALE, None, out_t.data_ptr(), 1024, 16 * 1024, 0)
    assert rc == -1 and b"workspace" in L.lib().omg_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()) and bool((out_t == -7.25).all()), "a refused call launched something"


# ------------------------------------------------------------------ masked attention, head_dim 64
MH, MD = 4, 64
MSCALE = MD ** -0.5


def masked_case(dtype, B, T, seed):
    """q | k as two column blocks of one projection buffer (as the text enhancer's fused q | k rows), v apart; q, k at 1.6."""
    qk = randn(B, T, 2 * MH * MD, seed=seed, scale=1.6).to(dtype)
    v = randn(B, T, MH * MD, seed=seed + 1).to(dtype)
    return qk, v


def mask_of(kind, B, T, seed):
    if kind == "full":
        return torch.ones(B, T, T, dtype=torch.bool)
    eye = torch.eye(T, dtype=torch.bool)[None].expand(B, T, T).clone()
    if kind == "diag":
        return eye
    # GroundingDINO's block mask: phrases attend inside themselves, special tokens to themselves only
    m = eye
    g = torch.Generator().manual_seed(seed)
    for b in range(B):
        s = 1
        while s < T - 1:
            e = min(T - 1, s + int(torch.randint(1, 9, (1,), generator=g)))
            m[b, s:e, s:e] = True
            s = e + 1
    return m


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("kind", ["block", "diag", "full"])
@pytest.mark.parametrize("T", [1, 11, 37, 64, 65, 256])
def test_attn_masked_against_float64(dev, T, kind, B, dtype):
    qk, v = masked_case(dtype, B, T, seed=T + 3)
    mask = mask_of(kind, B, T, seed=T)
    hd = MH * MD
    qk_d = qk.to(dev)
    out = ops.attn_masked(qk_d[..., :hd], qk_d[..., hd:], v.to(dev), MH, MSCALE, mask=mask.to(dev))
    q, k, vh = heads_of(qk[..., :hd], MH, MD), heads_of(qk[..., hd:], MH, MD), heads_of(v, MH, MD)
    keep = mask[:, None]
    bounded(f"attn-masked {_id(dtype)} T{T} {kind} B{B}", dtype, out, merged(truth_masked(q, k, vh, MSCALE, keep)),
            merged(model_masked(q, k, vh, MSCALE, keep)))
    if kind == "diag":          # a row that sees itself only is its own value row, bit for bit
        assert torch.equal(out.cpu().view(torch.int16), v.view(torch.int16))
    if kind == "full":          # and no mask is the full mask
        again = ops.attn_masked(qk_d[..., :hd], qk_d[..., hd:], v.to(dev), MH, MSCALE)
        assert torch.equal(again, out)


def test_attn_masked_rectangular_batched_equals_single_and_canaries(dev):
    B, Nq, Nk, hd = 2, 70, 37, MH * MD
    q = randn(B, Nq, hd, seed=71, scale=1.6).to(F16)
    k = randn(B, Nk, hd, seed=72, scale=1.6).to(F16)
    v = randn(B, Nk, hd, seed=73).to(F16)
    mask = rand(B, Nq, Nk, seed=74) > 0.4
    mask[:, :, 0] = True
    q_d, k_d, v_d, m_d = q.to(dev), k.to(dev), v.to(dev), mask.to(dev)
    buf = torch.full((B, Nq + 1, hd + 8), -7.25, dtype=F16, device=dev)
    out = ops.attn_masked(q_d, k_d, v_d, MH, MSCALE, mask=m_d, out=buf[:, :Nq, :hd])
    keep = mask[:, None]
    qh, kh, vh = heads_of(q, MH, MD), heads_of(k, MH, MD), heads_of(v, MH, MD)
    bounded("attn-masked 70x37", F16, out, merged(truth_masked(qh, kh, vh, MSCALE, keep)), merged(model_masked(qh, kh, vh, MSCALE, keep)))
    assert bool((buf[:, Nq:] == -7.25).all()) and bool((buf[:, :, hd:] == -7.25).all())
    one = ops.attn_masked(q_d[1:], k_d[1:], v_d[1:], MH, MSCALE, mask=m_d[1:])
    assert torch.equal(out[1:], one)


def test_attn_masked_rejects_what_it_cannot_run(dev):
    q = torch.zeros(1, 257, MH * MD, dtype=F16, device=dev)
    out = torch.full((1, 257, MH * MD), -7.25, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError, match="at most 256"):
        ops.attn_masked(q, q, q, MH, MSCALE, out=out)
    with pytest.raises(L.OmgHipError, match="dtype"):
        ops.attn_masked(q.float(), q.float(), q.float(), MH, MSCALE)
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()), "a refused call launched something"
