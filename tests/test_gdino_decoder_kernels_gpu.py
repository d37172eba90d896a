"""omg_attn_hd32, omg_msdeform_attn_box (csrc/gdino.hip), omg_gdino_contrastive and omg_gdino_ref_step (csrc/gdino_decoder.hip) against
float64 compositions of the same 16-bit operands (-m gpu), at the smallest shapes at which each can go wrong.

Attention at head_dim 32.  The rule, the constants C_MAX = C_RMS = 4 and `model_masked` of tests/test_gdino_kernels_gpu.py, redefined
here: exact scores on the 16-bit operands, P = round16(exp2(S - rowmax)), O = P v / sum(P) with the sum on the rounded P.

Deformable attention with box references.  The reference is the library's composition in float64 (softmax of the logits,
loc = c + off / 4 * (w, h) * 0.5, grid_sample per level, the weighted sum); the bound has the form of the point kernel's,

    |out - r| <= u16 |r| + E32 (1 + u16) + tiny,     E32 = 2^-24 vmax (K_SOFTMAX + K_SUM + K_COORD)

with K_SOFTMAX = 5 A + 24 and K_SUM = 64 as derived there (the softmax and the sum are the same code) and the coordinate term
re-derived for the box product.  The kernel forms the pixel coordinate as

    s = fl(w (W / 8))                  W / 8 is exact; one rounding, relative 2^-24
    x = fma(cx, W, fma(off, s, -0.5))  two roundings

A corner contributes only while -1 < x < W, and 0 <= cx <= 1 (a sigmoid times a valid ratio), so wherever the result depends on x
|off s| <= 2 W + 2.5: the rounding of s moves x by at most (2 W + 2.5) u, the inner fma rounds a value of at most 2 W + 3, the outer one
a value of at most W + 2: (5 W + 7.5) u in all, u = 2^-24.  The sampled value is continuous and piecewise bilinear in the coordinate
with slope at most 2 vmax (zero padding included), for x and for y:

    K_COORD = 4 (5 Dmax + 7.5),        Dmax = the largest level side.

The measured maximum of |out - r| / bound is printed beside the bound.

Contrastive scores.  float64 on the 16-bit operands; the products are exact in fp32, the 256-term fp32 sum is within
256 2^-24 sum |x y| of it whatever its order.

Reference step.  float64 evaluation of the library's formula on the same fp32 / 16-bit inputs.  The embedding: one ulp of the storage
type at 1.0 (2^-10 fp16, 2^-7 bf16).  ref_out / ref_input: 4 x the maximum error of torch's own fp32 evaluation of the same formula on
the same inputs against float64 (the kernel sums the 256-term product in another order).
Measured on MI355X: kernel error / torch fp32 error = 0.49 .. 1.08 over the cases below (printed by the test; both errors are
0.8e-7 .. 2.6e-7, the embedding's 2.44e-4 fp16 / 1.95e-3 bf16, a quarter of the allowed ulp).
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
HEADS = 8


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


# ------------------------------------------------------------------ attention at head_dim 32
AD = 32
ASCALE = AD ** -0.5
SIZES = [1, 15, 16, 17, 63, 64, 65, 70, 130]


def masked_scores(q, k, scale, keep):
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
    return t.reshape(t.shape[0], t.shape[1], heads, d).permute(0, 2, 1, 3)


def merged(t):
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)


def hd32_case(dtype, B, Nq, Nk, seed):
    """q | k as column blocks of one projection buffer where Nq == Nk (the decoder's fused rows), else apart; q, k at 1.5."""
    hd = HEADS * AD
    q = randn(B, Nq, hd, seed=seed, scale=1.5).to(dtype)
    k = randn(B, Nk, hd, seed=seed + 1, scale=1.5).to(dtype)
    v = randn(B, Nk, hd, seed=seed + 2).to(dtype)
    return q, k, v


def key_mask_of(kind, B, Nk, seed):
    """none | scattered (about a third excluded, never everything) | tile (one whole 64-key tile excluded, or the first half of the only one)"""
    if kind == "none":
        return None
    m = rand(B, Nk, seed=seed) > 0.35
    m[:, Nk - 1] = True
    if kind == "tile":
        m[:] = True
        if Nk > 64:
            m[:, :64] = False
        else:
            m[:, :Nk // 2] = False
    return m


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("kind", ["none", "scattered", "tile"])
@pytest.mark.parametrize("Nk", SIZES)
@pytest.mark.parametrize("Nq", SIZES)
def test_attn_hd32_against_float64(dev, Nq, Nk, kind, dtype):
    B = 2
    q, k, v = hd32_case(dtype, B, Nq, Nk, seed=Nq * 131 + Nk)
    km = key_mask_of(kind, B, Nk, seed=Nq + Nk)
    out = ops.attn_hd32(q.to(dev), k.to(dev), v.to(dev), HEADS, ASCALE, key_mask=None if km is None else km.to(dev))
    qh, kh, vh = heads_of(q, HEADS, AD), heads_of(k, HEADS, AD), heads_of(v, HEADS, AD)
    keep = None if km is None else km[:, None, None, :]
    bounded(f"attn-hd32 {_id(dtype)} {Nq}x{Nk} {kind}", dtype, out, merged(truth_masked(qh, kh, vh, ASCALE, keep)),
            merged(model_masked(qh, kh, vh, ASCALE, keep)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("NN", [(70, 130), (17, 65)], ids=_id)
def test_attn_hd32_equal_scores_give_the_mean_of_v(dev, NN, dtype):
    """q = 0: every probability is equal; v on the grid of eighths, so the sums are exact: one rounding of the mean over the keys that
    take part."""
    Nq, Nk = NN
    B, hd = 2, HEADS * AD
    q, k, _ = hd32_case(dtype, B, Nq, Nk, seed=3)
    q[:] = 0
    v = (torch.round(randn(B, Nk, hd, seed=4) * 8.0) / 8.0).to(dtype)
    km = key_mask_of("tile", B, Nk, seed=5)
    out = ops.attn_hd32(q.to(dev), k.to(dev), v.to(dev), HEADS, ASCALE, key_mask=km.to(dev)).double().cpu()
    for b in range(B):
        want = v[b, km[b]].double().mean(0)
        assert float((out[b] - want).abs().max()) <= M.ulp(dtype) * float(want.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_attn_hd32_dominant_key_gives_its_value_row(dev, dtype):
    """Row r's query is 16 x the key j(r): its score is far above every other one, the other probabilities round to zero: the output is
    the key's value row, bit for bit."""
    B, Nq, Nk, hd = 1, 70, 130, HEADS * AD
    q, k, v = hd32_case(dtype, B, Nq, Nk, seed=6)
    j = torch.randint(0, Nk, (Nq,), generator=torch.Generator().manual_seed(7))
    q[0] = (k[0, j].float() * 16.0).to(dtype)
    out = ops.attn_hd32(q.to(dev), k.to(dev), v.to(dev), HEADS, ASCALE).cpu()
    assert torch.equal(out[0].view(torch.int16), v[0, j].contiguous().view(torch.int16))


def test_attn_hd32_strides_canaries_and_batched_equals_single(dev):
    B, Nq, Nk, hd = 2, 70, 70, HEADS * AD
    q, k, v = hd32_case(F16, B, Nq, Nk, seed=8)
    km = key_mask_of("scattered", B, Nk, seed=9).to(dev)
    dense = ops.attn_hd32(q.to(dev), k.to(dev), v.to(dev), HEADS, ASCALE, key_mask=km)
    # q | k | v as column slices of one fused buffer with padded rows, a canary-filled output with padded rows and samples
    fused = torch.zeros(B, Nq + 2, 3 * hd + 8, dtype=F16, device=dev)
    fused[:, :Nq, :hd], fused[:, :Nq, hd:2 * hd], fused[:, :Nq, 2 * hd:3 * hd] = q.to(dev), k.to(dev), v.to(dev)
    buf = torch.full((B, Nq + 1, hd + 8), -7.25, dtype=F16, device=dev)
    ops.attn_hd32(fused[:, :Nq, :hd], fused[:, :Nq, hd:2 * hd], fused[:, :Nq, 2 * hd:3 * hd], HEADS, ASCALE, key_mask=km, out=buf[:, :Nq, :hd])
    assert torch.equal(buf[:, :Nq, :hd], dense) and bool((buf[:, Nq:] == -7.25).all()) and bool((buf[:, :, hd:] == -7.25).all())
    one = ops.attn_hd32(q[1:].to(dev), k[1:].to(dev), v[1:].to(dev), HEADS, ASCALE, key_mask=km[1:])
    assert torch.equal(dense[1:], one)
    # a mask of ones is no mask
    a = ops.attn_hd32(q.to(dev), k.to(dev), v.to(dev), HEADS, ASCALE, key_mask=torch.ones(B, Nk, dtype=torch.bool, device=dev))
    assert torch.equal(a, ops.attn_hd32(q.to(dev), k.to(dev), v.to(dev), HEADS, ASCALE))


def test_attn_hd32_rejects_what_it_cannot_run(dev):
    q = torch.zeros(1, 8, HEADS * AD, dtype=F16, device=dev)
    out = torch.full((1, 8, HEADS * AD), -7.25, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError, match="dtype"):
        ops.attn_hd32(q.float(), q.float(), q.float(), HEADS, ASCALE)
    lib = L.lib()
    rc = lib.omg_attn_hd32(L.OMG_F16, 1, HEADS, 8, 8, q.data_ptr() + 2, 256, 2048, q.data_ptr(), 256, 2048, q.data_ptr(), 256, 2048, None,
                           ASCALE, out.data_ptr(), 256, 2048, None)
    assert rc == -1 and b"aligned" in lib.omg_last_error()
    rc = lib.omg_attn_hd32(L.OMG_F16, 1, HEADS, 8, 8, q.data_ptr(), 252, 2048, q.data_ptr(), 256, 2048, q.data_ptr(), 256, 2048, None,
                           ASCALE, out.data_ptr(), 256, 2048, None)
    assert rc == -1 and b"row stride" in lib.omg_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()), "a refused call launched something"


# ------------------------------------------------------------------ deformable attention with box references
LEVELS4 = [(13, 19), (7, 10), (4, 5), (2, 3)]
BOX_SHAPES = [LEVELS4, [(1, 1)], [(1, 7)], [(5, 1)]]


def starts_of(shapes):
    out, s = [], 0
    for h, w in shapes:
        out.append(s)
        s += h * w
    return out, s


def box_case(dtype, B, shapes, Nq, seed, with_mask):
    """value N(0, 1); logits N(0, 2.5^2); offsets N(0, 2^2) (units of an eighth of the box); centres uniform in [0, 1], sizes uniform in
    [0, 0.6].  Queries 0 .. 5 of every sample are the special boxes: zero size (every point on the centre), reaching far outside on
    either side, ref exactly 0 and exactly 1, centres on pixel centres."""
    Lv = len(shapes)
    _, N = starts_of(shapes)
    value = randn(B, N, HEADS * 32, seed=seed)
    off = randn(B, Nq, HEADS, Lv, 4, 2, seed=seed + 1, scale=2.0)
    lg = randn(B, Nq, HEADS, Lv * 4, seed=seed + 2, scale=2.5)
    ref = rand(B, Nq, Lv, 4, seed=seed + 3)
    ref[..., 2:] *= 0.6
    for q in range(min(Nq, 6)):
        if q == 0:
            ref[:, q, :, 2:] = 0.0
        elif q == 1:
            ref[:, q, :, 2:], off[:, q] = 1.0, 1000.0
        elif q == 2:
            ref[:, q, :, 2:], off[:, q] = 1.0, -1000.0
        elif q == 3:
            ref[:, q] = 0.0
        elif q == 4:
            ref[:, q] = 1.0
        else:                                   # centre on a pixel centre, zero size: the pixel coordinate is an integer exactly
            for l, (h, w) in enumerate(shapes):
                ref[:, q, l, 0], ref[:, q, l, 1] = (w // 2 + 0.5) / w, (h // 2 + 0.5) / h
            ref[:, q, :, 2:] = 0.0
    ow = torch.cat([off.reshape(B, Nq, -1), lg.reshape(B, Nq, -1)], dim=-1).to(dtype)
    mask = None
    if with_mask:
        mask = rand(B, N, seed=seed + 9) > 0.3
        mask[:, 0] = True                       # never everything (a level of one row)
    return value.to(dtype), ow, ref, mask


def sample_truth(value, ow, loc, shapes, mask):
    """float64, as multi_scale_deformable_attention composes it, from sampling locations [B, Nq, heads, L, 4, 2]: [B, Nq, heads 32]."""
    B, N, _ = value.shape
    Nq, Lv = ow.shape[1], len(shapes)
    v = value.double()
    if mask is not None:
        v = v.masked_fill(~mask[..., None], 0.0)
    v = v.view(B, N, HEADS, 32)
    a = torch.softmax(ow.double()[..., HEADS * Lv * 8:].view(B, Nq, HEADS, Lv * 4), dim=-1).view(B, Nq, HEADS, Lv, 4)
    grids = 2.0 * loc - 1.0
    starts, _ = starts_of(shapes)
    out = torch.zeros(B * HEADS, 32, Nq, dtype=torch.float64)
    for l, (h, w) in enumerate(shapes):
        vl = v[:, starts[l]:starts[l] + h * w].permute(0, 2, 3, 1).reshape(B * HEADS, 32, h, w)
        gl = grids[:, :, :, l].transpose(1, 2).reshape(B * HEADS, Nq, 4, 2)
        s = F.grid_sample(vl, gl, mode="bilinear", padding_mode="zeros", align_corners=False)
        al = a[:, :, :, l].transpose(1, 2).reshape(B * HEADS, 1, Nq, 4)
        out += (s * al).sum(-1)
    return out.view(B, HEADS, 32, Nq).permute(0, 3, 1, 2).reshape(B, Nq, HEADS * 32)


def offsets_of(ow, Lv):
    B, Nq = ow.shape[:2]
    return ow.double()[..., :HEADS * Lv * 8].view(B, Nq, HEADS, Lv, 4, 2)


def box_truth(value, ow, ref, shapes, mask):
    r = ref.double()
    loc = r[:, :, None, :, None, :2] + offsets_of(ow, len(shapes)) / 4 * r[:, :, None, :, None, 2:] * 0.5
    return sample_truth(value, ow, loc, shapes, mask)


def point_truth(value, ow, ref, shapes, mask):
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    loc = ref.double()[:, :, None, :, None, :] + offsets_of(ow, len(shapes)) / norm[None, None, None, :, None, :]
    return sample_truth(value, ow, loc, shapes, mask)


def msd_bound(dtype, truth, value, ow, shapes, k_coord):
    Lv = len(shapes)
    u16 = 2.0 ** -11 if dtype == F16 else 2.0 ** -8
    vmax = float(value.double().abs().max())
    A = LOG2E * float(ow[..., HEADS * Lv * 8:].double().abs().max())
    k = (5.0 * A + 24.0) + 64.0 + k_coord
    e32 = 2.0 ** -24 * vmax * k
    return u16 * truth.abs() + e32 * (1.0 + u16) + 2.0 ** -25, k


def k_coord_box(shapes):
    return 4.0 * (5.0 * max(max(s) for s in shapes) + 7.5)


def run_box(dev, value, ow, ref, shapes, mask, **kw):
    return ops.msdeform_attn_box(value.to(dev), ow.to(dev), ref.to(dev), shapes, heads=HEADS, mask=None if mask is None else mask.to(dev), **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shapes", BOX_SHAPES, ids=_id)
def test_msdeform_box_against_float64(dev, shapes, with_mask, dtype):
    B = 2
    _, N = starts_of(shapes)
    Nq = 70 if len(shapes) == 4 else 37
    value, ow, ref, mask = box_case(dtype, B, shapes, Nq, seed=N * 5 + 1, with_mask=with_mask)
    out = run_box(dev, value, ow, ref, shapes, mask)
    truth = box_truth(value, ow, ref, shapes, mask)
    bound, k = msd_bound(dtype, truth, value, ow, shapes, k_coord_box(shapes))
    err = (out.double().cpu() - truth).abs()
    ratio = float((err / bound).max())
    print(f"msdeform-box {_id(dtype)} {_id(shapes)} mask{int(with_mask)}: K = {k:.0f}, max err {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    assert bool(torch.isfinite(out).all())
    assert float(truth.abs().max()) > 0.1
    # a box of zero size samples its centre with every point: the far-out boxes sample nothing
    assert float(truth[:, 1:3].abs().max()) == 0.0 and bool((out[:, 1:3] == 0).all())
    assert ratio <= 1.0, f"max |out - truth| / bound = {ratio:.3f}"


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_msdeform_box_of_eight_pixels_is_the_point_form(dev, dtype):
    """A box of w = 8 / W_l, h = 8 / H_l steps one pixel per unit of offset, as the point form does.  Where 8 / W_l is a binary fraction
    the step s is exactly 1 and the two kernels do the same arithmetic: bit for bit.  On the model's level set fl(8 / W_l) carries one
    more rounding than the derivation above counts (another (2 W + 2.5) u on the coordinate): within the bound with
    K_COORD = 4 (7 Dmax + 10) of the POINT form's float64 value, and so is omg_msdeform_attn itself."""
    B, Nq = 2, 70
    for shapes, exact in (([(8, 16), (4, 8), (2, 4), (1, 2)], True), (LEVELS4, False)):
        value, ow, ref, mask = box_case(dtype, B, shapes, Nq, seed=31, with_mask=True)
        for l, (h, w) in enumerate(shapes):
            ref[:, :, l, 2], ref[:, :, l, 3] = 8.0 / w, 8.0 / h
        box = run_box(dev, value, ow, ref, shapes, mask)
        pts = ref[..., :2].contiguous()
        point = ops.msdeform_attn(value.to(dev), ow.to(dev), pts.to(dev), shapes, heads=HEADS, mask=mask.to(dev))
        if exact:
            assert torch.equal(box.view(torch.int16), point.view(torch.int16))
            continue
        truth = point_truth(value, ow, pts, shapes, mask)
        bound, _ = msd_bound(dtype, truth, value, ow, shapes, 4.0 * (7.0 * 19 + 10.0))
        for name, o in (("box", box), ("point", point)):
            ratio = float(((o.double().cpu() - truth).abs() / bound).max())
            print(f"msdeform-box as points {_id(dtype)} {name}: max err / bound {ratio:.3f}")
            assert ratio <= 1.0, (name, ratio)


def test_msdeform_box_strides_canaries_and_batched_equals_single(dev):
    shapes = LEVELS4
    _, N = starts_of(shapes)
    B, Nq = 2, 70
    value, ow, ref, mask = box_case(F16, B, shapes, Nq, seed=41, with_mask=True)
    dense = run_box(dev, value, ow, ref, shapes, mask)
    buf = torch.full((B * Nq + 3, 256 + 8), -7.25, dtype=F16, device=dev)
    got = run_box(dev, value, ow, ref, shapes, mask, out=buf[:B * Nq].view(B, Nq, 264))
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:B * Nq, :256].reshape(B, Nq, 256).view(torch.int16), dense.view(torch.int16))
    assert bool((buf[:B * Nq, 256:] == -7.25).all()) and bool((buf[B * Nq:] == -7.25).all())
    # the value as a column slice of a stacked projection (six layers' value_proj side by side)
    wide_v = torch.zeros(B, N, 6 * 256, dtype=F16, device=dev)
    wide_v[..., 512:768] = value.to(dev)
    wide_ow = torch.zeros(B, Nq, 384 + 8, dtype=F16, device=dev)
    wide_ow[..., :384] = ow.to(dev)
    again = ops.msdeform_attn_box(wide_v[..., 512:768], wide_ow[..., :384], ref.to(dev), shapes, heads=HEADS, mask=mask.to(dev))
    assert torch.equal(again.view(torch.int16), dense.view(torch.int16))
    one = run_box(dev, value[1:], ow[1:], ref[1:], shapes, mask[1:])
    assert torch.equal(dense[1:], one)
    # every value row masked: zeros, bit for bit
    z = run_box(dev, value, ow, ref, shapes, torch.zeros(B, N, dtype=torch.bool)).cpu()
    assert bool((z.view(torch.int16) == 0).all())


def test_msdeform_box_rejects_what_it_cannot_run(dev):
    shapes = LEVELS4
    value, ow, ref, _ = box_case(F16, 1, shapes, 8, seed=51, with_mask=False)
    out = torch.full((1, 8, 256), -7.25, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError, match="beyond N"):
        ops.msdeform_attn_box(value.to(dev), ow.to(dev), ref.to(dev), shapes, heads=HEADS, level_start=[0, 247, 317, 338], out=out)
    with pytest.raises(L.OmgHipError, match="levels"):
        ops.msdeform_attn_box(value.to(dev), ow.to(dev), ref.to(dev).repeat(1, 1, 2, 1)[:, :, :5].contiguous(), shapes + [(1, 1)], heads=HEADS, out=out)
    with pytest.raises(AssertionError):                     # point references are not box references
        ops.msdeform_attn_box(value.to(dev), ow.to(dev), ref.to(dev)[..., :2].contiguous(), shapes, heads=HEADS, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()), "a refused call launched something"


# ------------------------------------------------------------------ contrastive scores
def contrastive_case(dtype, B, N, T, seed):
    x = randn(B, N, 256, seed=seed).to(dtype)
    y = randn(B, T, 256, seed=seed + 1).to(dtype)
    m = rand(B, T, seed=seed + 2) > 0.3
    m[:, 0] = True                              # [CLS]
    return x, y, m


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("T", [1, 11, 37, 256])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 343])
def test_contrastive_against_float64(dev, N, T, dtype):
    B, MT = 2, 256
    x, y, m = contrastive_case(dtype, B, N, T, seed=N * 3 + T)
    lg, rm = ops.gdino_contrastive(x.to(dev), y.to(dev), m.to(dev), MT, logits=True, rowmax=True)
    only = ops.gdino_contrastive(x.to(dev), y.to(dev), m.to(dev), MT, logits=False, rowmax=True)
    lg, rm, only = lg.cpu(), rm.cpu(), only.cpu()
    assert lg.shape == (B, N, MT) and lg.dtype == torch.float32 and rm.shape == (B, N)
    keep = torch.zeros(B, N, MT, dtype=torch.bool)
    keep[:, :, :T] = m[:, None, :]
    assert torch.equal(torch.isneginf(lg), ~keep), "-inf exactly on masked tokens and beyond T"
    truth = x.double() @ y.double().transpose(1, 2)
    bound = 256 * 2.0 ** -24 * (x.double().abs() @ y.double().abs().transpose(1, 2))
    err = (lg[:, :, :T].double() - truth).abs()
    ratio = float((err / bound)[keep[:, :, :T]].max())
    print(f"contrastive {_id(dtype)} N{N} T{T}: max err / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(rm.view(torch.int32), lg.max(-1)[0].view(torch.int32)), "rowmax is the maximum of the logits, bit for bit"
    assert torch.equal(only.view(torch.int32), rm.view(torch.int32)), "and the same without the logits"


def test_contrastive_strides_max_text_len_and_batched_equals_single(dev):
    B, N, T = 2, 70, 37
    x, y, m = contrastive_case(F16, B, N, T, seed=5)
    lg = ops.gdino_contrastive(x.to(dev), y.to(dev), m.to(dev), 256)
    wx = torch.zeros(B, N, 264, dtype=F16, device=dev)
    wx[..., :256] = x.to(dev)
    wy = torch.zeros(B, T, 512, dtype=F16, device=dev)
    wy[..., 256:] = y.to(dev)
    assert torch.equal(ops.gdino_contrastive(wx[..., :256], wy[..., 256:], m.to(dev), 256), lg)
    one = ops.gdino_contrastive(x[1:].to(dev), y[1:].to(dev), m[1:].to(dev), 256)
    assert torch.equal(lg[1:], one)
    short = ops.gdino_contrastive(x.to(dev), y.to(dev), m.to(dev), 40)
    assert short.shape == (B, N, 40) and torch.equal(short, lg[..., :40])
    with pytest.raises(L.OmgHipError, match="max_text_len"):
        ops.gdino_contrastive(x.to(dev), y.to(dev), m.to(dev), 36)
    with pytest.raises(L.OmgHipError, match="max_text_len"):
        ops.gdino_contrastive(x.to(dev), y.to(dev), m.to(dev), 260)


# ------------------------------------------------------------------ the reference step
def sine_embed64(pos):
    """encode_sinusoidal_position_embedding in float64 on the fp32 coordinates [.., 4] (x, y, w, h) -> [.., 512]: y, x, w, h."""
    dim_t = torch.arange(128, dtype=torch.float64)
    dim_t = 10000.0 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / 128)
    es = []
    for c in pos.double().unbind(-1):
        e = c[..., None] * (2 * math.pi) / dim_t
        es.append(torch.stack((e[..., 0::2].sin(), e[..., 1::2].cos()), dim=-1).flatten(-2))
    es[0], es[1] = es[1], es[0]
    return torch.cat(es, dim=-1)


def ref_formula(ref_in, logit_in, hidden, w3, b3, vr, dt):
    """The library's formula at precision dt (float64 truth, float32: torch's own evaluation): (ref_out, ref_input)."""
    base = logit_in.to(dt) if logit_in is not None else torch.special.logit(ref_in.to(dt), eps=1e-5)
    if hidden is not None:
        out = (hidden.to(dt) @ w3.to(dt).t() + b3.to(dt) + base).sigmoid()
    else:
        out = ref_in.to(dt) if ref_in is not None else base.sigmoid()
    return out, out[:, :, None] * torch.cat([vr, vr], -1).to(dt)[:, None]


def ref_case(dtype, B, Q, Lv, seed):
    ref = rand(B, Q, 4, seed=seed)
    ref[:, 0], ref[:, 1], ref[:, 2], ref[:, 3] = 0.0, 1.0, 1e-7, 1.0 - 1e-7
    hidden = torch.relu(randn(B, Q, 256, seed=seed + 1)).to(dtype)
    w3 = randn(4, 256, seed=seed + 2, scale=0.1).to(dtype)
    b3 = randn(4, seed=seed + 3, scale=0.5).to(dtype)
    vr = 0.5 + 0.5 * rand(B, Lv, 2, seed=seed + 4)
    vr[0] = 1.0
    return ref, hidden, w3, b3, vr


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("mode", ["layer", "first", "selection"])
@pytest.mark.parametrize("Lv", [4, 1])
def test_ref_step_against_float64(dev, Lv, mode, dtype):
    B, Q = 2, 70
    ref, hidden, w3, b3, vr = ref_case(dtype, B, Q, Lv, seed=Lv + 11)
    ref_in, logit_in, hid = ref, None, hidden
    if mode == "first":
        hid = None
    if mode == "selection":
        ref_in, logit_in = None, torch.log(ref / (1 - ref))          # the proposals' inverse sigmoid: +inf at 1, -inf at 0
        logit_in[:, 5] = float("inf")                                # an invalid proposal
    kw = dict(ref_in=None if ref_in is None else ref_in.to(dev), logit_in=None if logit_in is None else logit_in.to(dev), dtype=dtype)
    if hid is not None:
        kw.update(hidden=hid.to(dev), w3=w3.to(dev), b3=b3.to(dev))
    out, inp, emb = ops.gdino_ref_step(vr.to(dev), **kw)
    out, inp, emb = out.cpu(), inp.cpu(), emb.cpu()
    t_out, t_inp = ref_formula(ref_in, logit_in, hid, w3, b3, vr, torch.float64)
    f_out, f_inp = ref_formula(ref_in, logit_in, hid, w3, b3, vr, torch.float32)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(emb).all())
    if mode == "first":
        assert torch.equal(out, ref), "the step in front of layer 0 passes the reference through"
    if mode == "selection":
        assert bool((out[:, 5] == 1.0).all()), "sigmoid(delta + inf) = 1"
    for name, got, tr, fl in (("ref_out", out, t_out, f_out), ("ref_input", inp, t_inp, f_inp)):
        e_k, e_t = float((got.double() - tr).abs().max()), float((fl.double() - tr).abs().max())
        print(f"ref_step {_id(dtype)} {mode} L{Lv} {name}: kernel {e_k:.3e}, torch fp32 {e_t:.3e}, ratio {e_k / max(e_t, 1e-30):.2f}")
        assert e_k <= 4.0 * e_t, (name, e_k, e_t)
    want = sine_embed64(inp[:, :, 0])                              # the kernel's own fp32 ref_input, as the library embeds its own
    ulp1 = 2.0 ** -10 if dtype == F16 else 2.0 ** -7
    e = float((emb.double() - want).abs().max())
    print(f"ref_step {_id(dtype)} {mode} L{Lv} embedding: max err {e:.3e} (one ulp at 1.0: {ulp1:.3e})")
    assert e <= ulp1
    # the channel order: y before x, then w, h (a swapped pair of blocks is an error of order 1)
    swapped = torch.cat([want[..., 128:256], want[..., :128], want[..., 256:]], -1)
    assert float((emb.double() - swapped).abs().max()) > 0.1


def test_ref_step_batched_equals_single_and_refusals(dev):
    B, Q, Lv = 2, 19, 4
    ref, hidden, w3, b3, vr = ref_case(F16, B, Q, Lv, seed=21)
    args = dict(hidden=hidden.to(dev), w3=w3.to(dev), b3=b3.to(dev))
    both = ops.gdino_ref_step(vr.to(dev), ref_in=ref.to(dev), **args)
    one = ops.gdino_ref_step(vr[1:].to(dev), ref_in=ref[1:].to(dev), hidden=hidden[1:].to(dev), w3=w3.to(dev), b3=b3.to(dev))
    for a, b in zip(both, one):
        assert torch.equal(a[1:], b)
    # the hidden state as a column slice with padded rows
    wide = torch.zeros(B, Q, 264, dtype=F16, device=dev)
    wide[..., :256] = hidden.to(dev)
    again = ops.gdino_ref_step(vr.to(dev), ref_in=ref.to(dev), hidden=wide[..., :256], w3=w3.to(dev), b3=b3.to(dev))
    for a, b in zip(both, again):
        assert torch.equal(a, b)
    lib = L.lib()
    r = ref.to(dev)
    rc = lib.omg_gdino_ref_step(L.OMG_F16, B, Q, Lv, r.data_ptr(), r.data_ptr(), vr.to(dev).data_ptr(), None, 0, None, None, r.data_ptr(), None, None, 0, None)
    assert rc == -1 and b"exactly one" in lib.omg_last_error()
    rc = lib.omg_gdino_ref_step(L.OMG_F16, B, Q, 5, r.data_ptr(), None, vr.to(dev).data_ptr(), None, 0, None, None, r.data_ptr(), None, None, 0, None)
    assert rc == -1 and b"levels" in lib.omg_last_error()
