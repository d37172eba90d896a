"""SAM's mask-decoder kernels on the GPU (-m gpu): omg_attn_small, omg_convt2x2_ln_gelu, omg_sam_mask_logits, omg_sam_postprocess
and omg_relu (csrc/sam_decoder.hip) against torch fp32 on the same 16-bit operands.

Tolerances follow tests/test_effvit_gpu.py: the same computation is done by torch on the GPU in the storage dtype, its error E against
the fp32 result is measured, and the HIP kernel is allowed 2 E (another accumulation order) plus one ulp of the storage dtype at the
output's largest magnitude.  Nothing absolute is fixed in advance.  With OMG_SAM_ERRORS_JSON=path the measured values are written
there when the module is done.  Cases with an exact answer (one-hot and uniform softmax, small integers) are compared bitwise."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from omg_amd import ops, sam
from tests import sam_torch as st
from tests.effvit_torch import seed_encoder
from tests.sam_torch import narrow_model

DTYPES = [torch.float16, torch.bfloat16]
MEASURED = {}
CANARY = 1234.0
NQ = [1, 7, 9, 65, 300]
NK = [1, 7, 63, 64, 65, 257, 4096]


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("OMG_SAM_ERRORS_JSON")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float16):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def ulp(dtype, mag):
    bits = 10 if dtype == torch.float16 else 7
    return 2.0 ** (math.floor(math.log2(max(mag, 2.0 ** -14))) - bits)


def name(dtype):
    return str(dtype)[6:]


def check(tag, dtype, got, ref32, torch16):
    """got, torch16: results of the kernel and of torch in the storage dtype (any device); ref32: fp32 on the CPU."""
    e_torch = (torch16.float().cpu() - ref32).abs().max().item()
    e_hip = (got.float().cpu() - ref32).abs().max().item()
    bound = 2.0 * e_torch + ulp(dtype, ref32.abs().max().item())
    MEASURED[tag] = {"torch_storage_dtype_err": e_torch, "hip_err": e_hip, "bound": bound, "max_abs_ref": ref32.abs().max().item()}
    print(f"{tag}: hip {e_hip:.3e}  torch-{name(dtype)} {e_torch:.3e}  bound {bound:.3e}")
    assert math.isfinite(e_hip) and e_hip <= bound, (tag, e_hip, bound)


# ------------------------------------------------------------------------------------------------ omg_attn_small
def heads_first(t, heads):
    B, N, Wd = t.shape
    return t.view(B, N, heads, Wd // heads).transpose(1, 2)


def attn_torch(q, k, v, heads, scale):
    """softmax(q k^T scale) v per head in the dtype of the operands; [B, N, heads * d] in and out."""
    qh, kh, vh = (heads_first(t, heads) for t in (q, k, v))
    p = torch.softmax((qh @ kh.transpose(-1, -2)) * scale, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(q.shape)


def strided(t, dev, pad_value=7.0):
    """``t`` [B, N, W] on the device as a column slice (offset 8) of a buffer 24 columns wider."""
    B, N, Wd = t.shape
    wide = torch.full((B, N, Wd + 24), pad_value, dtype=t.dtype)
    wide[:, :, 8:8 + Wd] = t
    return wide.to(dev)[:, :, 8:8 + Wd]


def run_attn(q, k, v, heads, scale, dev):
    """The kernel on strided operands into a canary-framed output; k and v are column slices of ONE buffer, as the decoder's are."""
    B, Nq, Wd = q.shape
    Nk = k.shape[1]
    kv = torch.full((B, Nk, 2 * Wd + 16), 7.0, dtype=q.dtype)
    kv[:, :, :Wd] = k
    kv[:, :, Wd + 8:2 * Wd + 8] = v
    kv = kv.to(dev)
    frame = torch.full((B * Nq + 1, Wd + 16), CANARY, dtype=q.dtype, device=dev)
    out = frame[:B * Nq].view(B, Nq, Wd + 16)[:, :, 8:8 + Wd]
    got = ops.attn_small(strided(q, dev), kv[:, :, :Wd], kv[:, :, Wd + 8:2 * Wd + 8], heads, scale, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.all(frame[:, :8] == CANARY) and torch.all(frame[:, 8 + Wd:] == CANARY) and torch.all(frame[B * Nq] == CANARY), "wrote outside the row"
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads", [1, 8])
@pytest.mark.parametrize("d", [16, 32])
def test_attn_small(dev, dtype, d, heads, B):
    """Every (Nq, Nk) of the grid: both kernels (keys over the lanes; a query per lane), partial last key tiles (63, 65, 257), one key, one
    query, more than one block of queries (65, 300)."""
    Wd = heads * d
    scale = d ** -0.5
    for Nk in NK:
        k, v = rnd(B, Nk, Wd, seed=2, dtype=dtype), rnd(B, Nk, Wd, seed=3, dtype=dtype)
        kd, vd = k.to(dev), v.to(dev)
        for Nq in NQ:
            q = rnd(B, Nq, Wd, seed=1, scale=2.0, dtype=dtype)
            ref32 = attn_torch(q.float(), k.float(), v.float(), heads, scale)
            t16 = attn_torch(q.to(dev), kd, vd, heads, scale)
            got = run_attn(q, k, v, heads, scale, dev)
            check(f"attn_small {name(dtype)} d{d} h{heads} B{B} Nq{Nq} Nk{Nk}", dtype, got, ref32, t16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 32])
@pytest.mark.parametrize("Nq,Nk", [(7, 64), (7, 4096), (65, 64), (300, 256)])
def test_attn_small_exact_answers(dev, dtype, d, Nq, Nk):
    """Softmax weights that are exactly representable: the result is known without a tolerance.  Nk is a power of two and V holds small
    integers, so every sum and the division are exact in fp32 and one rounding remains."""
    heads, B = 8, 2
    Wd = heads * d
    g = torch.Generator().manual_seed(11)
    v = torch.randint(-8, 9, (B, Nk, Wd), generator=g).to(dtype)
    mean = v.float().mean(dim=1, keepdim=True).expand(B, Nq, Wd).to(dtype)          # exact in fp32, rounded once

    # uniform scores (q = 0): the mean of V
    q0 = torch.zeros(B, Nq, Wd, dtype=dtype)
    k = rnd(B, Nk, Wd, seed=12, dtype=dtype)
    assert torch.equal(run_attn(q0, k, v, heads, d ** -0.5, dev).cpu(), mean)

    # all keys equal: every score of a row is the same non-zero number, the weights are uniform again
    q = rnd(B, Nq, Wd, seed=13, dtype=dtype)
    keq = k[:, :1].expand(B, Nk, Wd).contiguous()
    assert torch.equal(run_attn(q, keq, v, heads, d ** -0.5, dev).cpu(), mean)

    # one dominant key per (query, head): score 256 against 0, exp(-256) is 0 in fp32 -> one-hot, the result is that row of V
    star = torch.randint(0, Nk, (B, heads), generator=g)
    q1 = torch.zeros(B, Nq, heads, d)
    q1[..., 0] = 16.0
    k1 = torch.zeros(B, Nk, heads, d)
    want = torch.empty(B, Nq, heads, d)
    for b in range(B):
        for h in range(heads):
            k1[b, star[b, h], h, 0] = 16.0
            want[b, :, h] = v[b, star[b, h]].view(heads, d)[h].float()
    got = run_attn(q1.view(B, Nq, Wd).to(dtype), k1.view(B, Nk, Wd).to(dtype), v, heads, 1.0, dev)
    assert torch.equal(got.float().cpu(), want.view(B, Nq, Wd))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 32])
@pytest.mark.parametrize("Nq", [7, 300])
def test_attn_small_running_maximum_at_huge_scores(dev, dtype, d, Nq):
    """q . k = +-60000 (240 * 250: exact in both formats), scores +-60000 * scale: exp overflows without the running maximum and the
    maximum moves late, at the last four keys (for the split-key kernel: in four lanes out of 256, found only by the merge).  The answer is
    exactly the mean of those four rows of V."""
    heads, B, Nk = 8, 2, 1024
    Wd = heads * d
    scale = d ** -0.5
    g = torch.Generator().manual_seed(17)
    v = torch.randint(-8, 9, (B, Nk, Wd), generator=g).to(dtype)
    q = torch.zeros(B, Nq, heads, d)
    q[..., 0] = 240.0
    k = torch.zeros(B, Nk, heads, d)
    k[..., 0] = -250.0
    k[:, Nk - 4:, :, 0] = 250.0
    want = v[:, Nk - 4:].float().mean(dim=1, keepdim=True).expand(B, Nq, Wd)
    assert torch.equal(want, want.to(dtype).float())
    got = run_attn(q.view(B, Nq, Wd).to(dtype), k.view(B, Nk, Wd).to(dtype), v, heads, scale, dev)
    assert torch.equal(got.float().cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 32])
@pytest.mark.parametrize("Nq", [7, 300])
def test_attn_small_padded_key_tile_has_no_influence(dev, dtype, d, Nq):
    """65 keys = one full tile and one key of the next.  The same 65 keys inside a buffer whose rows 65.. are NaN give the same bits:
    nothing beyond Nk is weighted (0 * NaN would be NaN)."""
    heads, B, Nk = 8, 2, 65
    Wd = heads * d
    q, k, v = rnd(B, Nq, Wd, seed=21, dtype=dtype).to(dev), rnd(B, Nk, Wd, seed=22, dtype=dtype), rnd(B, Nk, Wd, seed=23, dtype=dtype)
    tight = ops.attn_small(q, k.to(dev), v.to(dev), heads, d ** -0.5)
    kb = torch.full((B, 192, Wd), float("nan"), dtype=dtype)
    vb = kb.clone()
    kb[:, :Nk], vb[:, :Nk] = k, v
    loose = ops.attn_small(q, kb.to(dev)[:, :Nk], vb.to(dev)[:, :Nk], heads, d ** -0.5)
    assert torch.isfinite(tight.float()).all() and torch.equal(tight, loose)


# ------------------------------------------------------------------------------------------------ omg_convt2x2_ln_gelu
def ln2d(x, w, b, eps=1e-6):
    """SAM's LayerNorm2d on NCHW."""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return w[:, None, None] * ((x - u) / torch.sqrt(s + eps)) + b[:, None, None]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (64, 64)])
@pytest.mark.parametrize("cin,cout", [(256, 64), (64, 32), (16, 8)])
def test_convt2x2_ln_gelu(dev, dtype, cin, cout, H, W, ln):
    """fp32 reference: F.conv_transpose2d on the CPU (so the weight packing and the scatter are checked against torch's own layout); the
    storage-dtype twin: the same GEMM by torch.matmul, bias, LayerNorm2d and GELU in the storage dtype."""
    B = 2
    x = rnd(B, cin, H, W, seed=31, dtype=dtype)
    w = rnd(cin, cout, 2, 2, seed=32, scale=cin ** -0.5, dtype=dtype)
    b = rnd(cout, seed=33, scale=0.5, dtype=dtype)
    lw, lb = (1.0 + 0.2 * rnd(cout, seed=34, dtype=torch.float32)).to(dtype), rnd(cout, seed=35, scale=0.2, dtype=dtype)
    pre32 = F.conv_transpose2d(x.float(), w.float(), b.float(), stride=2)
    ref32 = F.gelu(ln2d(pre32, lw.float(), lb.float()) if ln else pre32)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wp = ops.pack_convt2x2_weight(w).to(dev)
    rows = (xd.view(-1, cin) @ wp.t()).view(B, H, W, 2, 2, cout)
    pre16 = rows.permute(0, 5, 1, 3, 2, 4).reshape(B, cout, 2 * H, 2 * W) + b.to(dev)[:, None, None]
    t16 = F.gelu(ln2d(pre16, lw.to(dev), lb.to(dev)) if ln else pre16)
    frame = torch.full((B * 4 * H * W * cout + 2 * W * cout,), CANARY, dtype=dtype, device=dev)
    out = frame[:B * 4 * H * W * cout].view(B, 2 * H, 2 * W, cout)
    got = ops.convt2x2_ln_gelu(xd, wp, b.to(dev), ln_weight=lw.to(dev) if ln else None, ln_bias=lb.to(dev) if ln else None, out=out)
    assert torch.all(frame[out.numel():] == CANARY), "wrote past the output"
    check(f"convt2x2 {name(dtype)} {cin}->{cout} {H}x{W} ln{int(ln)}", dtype, got.permute(0, 3, 1, 2), ref32, t16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout", [(256, 64), (64, 32), (16, 8)])
def test_convt2x2_exact_on_small_integers(dev, dtype, cin, cout):
    g = torch.Generator().manual_seed(37)
    B, H, W = 2, 3, 5
    x = torch.randint(-1, 2, (B, cin, H, W), generator=g).float()
    w = torch.randint(-1, 2, (cin, cout, 2, 2), generator=g).float() * (torch.rand(cin, cout, 2, 2, generator=g) < 0.25)
    b = torch.randint(-4, 5, (cout,), generator=g).float()
    ref = F.conv_transpose2d(x, w, b, stride=2)
    assert torch.equal(ref, ref.to(dtype).float()) and ref.abs().max() >= 8, "the case itself must be exactly representable"
    got = ops.convt2x2_ln_gelu(x.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev), ops.pack_convt2x2_weight(w).to(dtype).to(dev),
                               b.to(dtype).to(dev), gelu=False)
    assert torch.equal(got.permute(0, 3, 1, 2).float().cpu(), ref)


# ------------------------------------------------------------------------------------------------ omg_sam_mask_logits
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("M", [1, 4])
def test_sam_mask_logits(dev, dtype, M, B):
    """The decoder's shape (256 x 256 pixels of 32 channels) and an odd one with a partial last block."""
    for (H, W) in [(256, 256), (5, 61)]:
        hyper, up = rnd(B, M, 32, seed=41, dtype=dtype), rnd(B, H, W, 32, seed=42, dtype=dtype)
        ref32 = torch.einsum("bmc,bhwc->bmhw", hyper.float(), up.float())
        t16 = torch.einsum("bmc,bhwc->bmhw", hyper.to(dev), up.to(dev))
        frame = torch.full((B * M * H * W + W,), CANARY, dtype=torch.float32, device=dev)
        out = frame[:B * M * H * W].view(B, M, H, W)
        got = ops.sam_mask_logits(hyper.to(dev), up.to(dev), out=out)
        assert got.dtype == torch.float32 and torch.all(frame[out.numel():] == CANARY), "wrote past the output"
        check(f"mask_logits {name(dtype)} M{M} B{B} {H}x{W}", dtype, got, ref32, t16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,B", [(1, 3), (4, 1), (3, 2)])
def test_sam_mask_logits_exact_on_small_integers(dev, dtype, M, B):
    g = torch.Generator().manual_seed(43)
    hyper = torch.randint(-3, 4, (B, M, 32), generator=g).float()
    up = torch.randint(-3, 4, (B, 16, 19, 32), generator=g).float()
    ref = torch.einsum("bmc,bhwc->bmhw", hyper, up)
    assert ref.abs().max() >= 32
    assert torch.equal(ops.sam_mask_logits(hyper.to(dtype).to(dev), up.to(dtype).to(dev)).cpu(), ref)


# ------------------------------------------------------------------------------------------------ omg_sam_postprocess
def postprocess_torch(low, image_size, input_size, original_size):
    """The reference's EfficientViTSam.postprocess_masks."""
    m = F.interpolate(low, (image_size, image_size), mode="bilinear", align_corners=False)
    m = m[..., :input_size[0], :input_size[1]]
    return F.interpolate(m, original_size, mode="bilinear", align_corners=False)


# (low-resolution side, image_size, input_size, original_size); the last is (1024 x 683 -> 1500 x 1000) at a quarter of the size
POST = [(256, 1024, (1024, 1024), (1024, 1024)), (256, 1024, (768, 1024), (96, 128)), (64, 256, (256, 171), (375, 250))]


@pytest.mark.parametrize("low_side,image_size,input_size,original_size", POST)
def test_sam_postprocess(dev, low_side, image_size, input_size, original_size):
    """fp32 logits against two F.interpolate calls in fp32 on the CPU, to fp32 rounding: each interpolation is three products-and-sums deep
    on values no larger than max |low| with weights in [0, 1], so either side is within 4 * 2^-24 * max |low| of the exact value per
    interpolation; two interpolations, two sides: 16 * 2^-24 * max |low|.  The uint8 mask equals the threshold of that reference
    except where the reference is within that rounding of the threshold; such pixels are at most 0.1 %, and the seeded input keeps the
    reference itself below that share."""
    B, M, thr = 2, 3, 0.0
    low = rnd(B, M, low_side, low_side, seed=51, scale=8.0, dtype=torch.float32)
    ref = postprocess_torch(low, image_size, input_size, original_size)
    tol = 16 * 2.0 ** -24 * low.abs().max().item()
    near = (ref - thr).abs() <= tol
    share = near.float().mean().item()
    assert share <= 1e-3, f"the reference itself has {share:.2%} of its pixels within rounding of the threshold"
    frame = torch.full((ref.numel() + original_size[1],), CANARY, dtype=torch.float32, device=dev)
    out = frame[:ref.numel()].view(ref.shape)
    got = ops.sam_postprocess(low.to(dev), image_size, input_size, original_size, out=out)
    assert torch.all(frame[ref.numel():] == CANARY), "wrote past the output"
    err = (got.cpu() - ref).abs().max().item()
    MEASURED[f"postprocess {low_side} {image_size} {input_size} {original_size}"] = {"hip_err": err, "bound": tol, "near_threshold_share": share}
    print(f"postprocess {input_size}->{original_size}: max |d| {err:.3e}  bound {tol:.3e}  near-threshold share {share:.2e}")
    assert err <= tol
    frame8 = torch.full((ref.numel() + original_size[1],), 77, dtype=torch.uint8, device=dev)
    out8 = frame8[:ref.numel()].view(ref.shape)
    mask = ops.sam_postprocess(low.to(dev), image_size, input_size, original_size, threshold=thr, out=out8)
    assert mask.dtype == torch.uint8 and torch.all(frame8[ref.numel():] == 77)
    mask = mask.cpu()
    assert int(mask.max()) <= 1
    differ = mask.bool() != (ref > thr)
    assert not (differ & ~near).any()
    assert torch.equal(mask.bool(), got.cpu() > thr)           # the two outputs of the kernel agree with each other everywhere


def test_sam_postprocess_threshold_is_strict_and_movable(dev):
    low = torch.full((1, 1, 8, 8), 0.5, device=dev)
    assert int(ops.sam_postprocess(low, 32, (32, 24), (16, 12), threshold=0.5).sum()) == 0       # a constant map stays constant; > is strict
    assert int(ops.sam_postprocess(low, 32, (32, 24), (16, 12), threshold=0.25).sum()) == 16 * 12


# ------------------------------------------------------------------------------------------------ omg_relu
@pytest.mark.parametrize("dtype", DTYPES)
def test_relu(dev, dtype):
    x = rnd(3, 7, 2048, seed=61, dtype=dtype).to(dev)
    assert torch.equal(ops.relu(x), torch.relu(x))
    y = x.clone()
    assert ops.relu(y, out=y).data_ptr() == y.data_ptr() and torch.equal(y, torch.relu(x))


# ================================================================================================ the modules and the predictor
# omg_amd.sam's prompt encoder, mask decoder and predictor against the fixture that the reference's own EfficientViTSam /
# EfficientViTSamPredictor produced in fp32 (tests/golden/sam_golden.npz, make_golden_sam.py).
#
# Per stage the convention is tests/test_effvit_gpu.py's for the narrow encoder (BASE and depths below restate it): max |d| / rms of the
# golden tensor below BASE sqrt(depth), depth = blocks in front of the tensor.  The prompt encoder is one rounding (depth 1); a two-way
# layer is four blocks (self-attention, token-to-image, MLP, image-to-token, each with its LayerNorm); the final attention one;
# output_upscaling two, the hypernetwork one and the mask product one; the IoU head one.  Masks are compared where the golden logit is
# further from the threshold than MULT x the measured low-resolution logit error of that image: the final logit is a convex (bilinear)
# combination of low-resolution logits, so its error cannot exceed theirs; the error is measured on every 4th pixel (the fixture's
# subsampling), which MULT = 2 (the fixture's cfg_mask_mult) covers.  The excluded share must stay <= 2 %.  The mask comparison runs in
# fp16, the predictor's default and the dtype the fixture's seed was chosen with; bf16 is compared per stage.
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_golden.npz")
BASE = {torch.float16: 3e-2, torch.bfloat16: 2e-1}          # tests/test_litemla_gpu.py: max |d| / rms against golden vectors, one block


def encoder_depth(cfg):
    """Blocks in front of the encoder's embedding, counted as tests/test_effvit_gpu.py counts them: the stem, every ResBlock /
    FusedMBConv / MBConv / LiteMLA, the neck's fusion, its middle blocks, its output convolution and the LayerNorm."""
    n = 1
    for s, dep in enumerate(cfg.depth_list):
        n += (1 if s else 0) + dep * (2 if cfg.block_list[s] == "att" else 1)
    return n + 1 + cfg.head_depth + 2


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def predictors(dev, gold):
    """dtype -> a predictor of the narrow model with the fixture's image set (built once, never modified by a test)."""
    out = {}
    for dt in DTYPES:
        p = sam.EfficientViTSamPredictor(narrow_model(gold, dt, dev))
        p.set_image(gold["image"])
        out[dt] = p
    return out


def stage(tag, dtype, got, ref, depth, failed):
    got, ref = got.float().cpu(), torch.as_tensor(ref).float()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    rel = (got - ref).abs().max().item() / ref.pow(2).mean().sqrt().item()
    bound = BASE[dtype] * math.sqrt(depth)
    MEASURED[f"{str(dtype)[6:]} {tag}"] = {"rel_err_max_over_rms": rel, "depth": depth, "bound": bound}
    print(f"narrow sam {str(dtype)[6:]} {tag}: max |d| / rms {rel:.3e}  (depth {depth}, bound {bound:.3e})")
    if not (math.isfinite(rel) and rel < bound):
        failed.append((tag, rel, bound))


@pytest.mark.parametrize("dtype", DTYPES)
def test_narrow_model_matches_the_reference_per_stage(dev, dtype, gold, predictors):
    p = predictors[dtype]
    m = p.model
    assert p.input_size == (192, 256) and p.original_size == (96, 128) and p.features.shape == (1, 64, 64, 256)
    sub, subk, subl = int(gold["cfg_sub_emb"]), int(gold["cfg_sub_keys"]), int(gold["cfg_sub_low"])
    d0 = encoder_depth(m.image_encoder.cfg)
    failed = []
    stage("features", dtype, p.features.permute(0, 3, 1, 2)[:, :, ::sub, ::sub], gold["features"], d0, failed)
    boxes = torch.as_tensor(gold["boxes_in"], dtype=torch.float, device=dev)
    sparse, dense = m.prompt_encoder(points=None, boxes=boxes, masks=None)
    stage("sparse (boxes)", dtype, sparse, gold["sparse_boxes"], 1, failed)
    stage("dense", dtype, dense, gold["dense"], 1, failed)
    pts = (torch.as_tensor(gold["points_in"], dtype=torch.float, device=dev)[None], torch.as_tensor(gold["point_labels"], dtype=torch.int, device=dev)[None])
    stage("sparse (points, padded)", dtype, m.prompt_encoder(points=pts, boxes=None, masks=None)[0], gold["sparse_points"], 1, failed)
    pe = m.prompt_encoder.get_dense_pe()
    assert pe is m.prompt_encoder.get_dense_pe()                                              # cached
    stage("dense_pe", dtype, pe.view(1, 64, 64, 256).permute(0, 3, 1, 2)[:, :, ::sub, ::sub], gold["dense_pe"], 1, failed)
    f = m.mask_decoder.forward_features(p.features, pe, sparse, dense, False)
    for i in range(2):
        stage(f"layer{i} queries", dtype, f[f"layer{i}_queries"], gold[f"layer{i}_queries"], d0 + 4 * (i + 1), failed)
        stage(f"layer{i} keys", dtype, f[f"layer{i}_keys"].view(3, 64, 64, 256)[:, ::subk, ::subk], gold[f"layer{i}_keys"], d0 + 4 * (i + 1), failed)
    stage("final queries", dtype, f["final_queries"], gold["final_queries"], d0 + 9, failed)
    assert f["masks"].dtype == torch.float32 and f["masks"].shape == (3, 1, 256, 256) and f["iou"].shape == (3, 1)
    stage("low-resolution logits", dtype, f["masks"][:, :, ::subl, ::subl], gold["low_boxes"], d0 + 13, failed)
    stage("iou", dtype, f["iou"], gold["iou_boxes"], d0 + 10, failed)
    fm = m.mask_decoder.forward_features(p.features, pe, sparse[:1], dense, True)
    stage("low-resolution logits, multimask", dtype, fm["masks"][:, :, ::subl, ::subl], gold["low_multi"], d0 + 13, failed)
    stage("iou, multimask", dtype, fm["iou"], gold["iou_multi"], d0 + 10, failed)
    assert not failed, failed


def masks_agree(tag, got_masks, gold_masks, gold_logits, err, mult):
    sel = np.abs(gold_logits) > mult * err
    excluded = 1.0 - sel.mean()
    wrong = int((got_masks[sel] != gold_masks[sel]).sum())
    MEASURED[f"float16 masks {tag}"] = {"low_res_logit_err": err, "excluded_share": excluded, "wrong_pixels": wrong, "area": float(gold_masks.mean())}
    print(f"masks {tag}: low-resolution logit error {err:.3e}, excluded share {excluded:.4f}, wrong among the rest {wrong}, golden area {gold_masks.mean():.3f}")
    assert wrong == 0 and excluded <= 0.02, (tag, wrong, excluded)


def test_final_masks_match_the_reference(dev, gold, predictors):
    p = predictors[torch.float16]
    mult, subl = float(gold["cfg_mask_mult"]), int(gold["cfg_sub_low"])
    boxes = torch.as_tensor(gold["boxes_in"], dtype=torch.float, device=dev)
    masks, iou, low = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)
    assert masks.dtype == torch.bool and masks.shape == (3, 1, 96, 128) and iou.shape == (3, 1) and low.shape == (3, 1, 256, 256)
    err = float((low[:, :, ::subl, ::subl].cpu() - torch.from_numpy(gold["low_boxes"])).abs().max())
    masks_agree("3 boxes", masks.cpu().numpy(), gold["masks_boxes"], gold["logits_boxes"], err, mult)
    logits = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False, return_logits=True)[0]
    assert logits.dtype == torch.float32 and torch.equal(logits > 0, masks)
    e_final = float((logits.cpu() - torch.from_numpy(gold["logits_boxes"])).abs().max())
    print(f"final logits: max |d| {e_final:.3e} (low-resolution {err:.3e})")
    assert e_final <= mult * err
    # predict(): numpy in the image's pixels, the two calls of the reference's OMG path
    m1, i1, l1 = p.predict(box=gold["boxes"][0], multimask_output=False)
    assert m1.dtype == np.bool_ and m1.shape == (1, 96, 128) and i1.shape == (1,) and l1.shape == (1, 256, 256) and l1.dtype == np.float32
    assert np.array_equal(m1, masks[0].cpu().numpy())
    masks_agree("predict(box)", m1, gold["masks_box_predict"], gold["logits_boxes"][0], err, mult)
    mp, ip, lp = p.predict(point_coords=gold["points"], point_labels=gold["point_labels"], multimask_output=True)
    assert mp.shape == (3, 96, 128) and ip.shape == (3,) and lp.shape == (3, 256, 256)
    failed = []
    d0 = encoder_depth(p.model.image_encoder.cfg)
    stage("predict(points) low-resolution logits", torch.float16, torch.from_numpy(lp[:, ::subl, ::subl]), gold["low_points"], d0 + 13, failed)
    stage("predict(points) iou", torch.float16, torch.from_numpy(ip), gold["iou_points"], d0 + 10, failed)
    assert not failed, failed
    # the second image: the host resize acts, another input_size
    q = sam.EfficientViTSamPredictor(p.model)
    q.set_image(gold["image_b"])
    assert q.input_size == (154, 256) and q.original_size == (60, 100)
    mb, _, lb = q.predict(box=gold["box_b"], multimask_output=False)
    err_b = float(np.abs(lb[:, ::subl, ::subl] - gold["low_b"]).max())
    masks_agree("image_b", mb, gold["masks_b"], gold["logits_b"], err_b, mult)


def test_batch_invariance_and_multimask_slices(dev, gold, predictors):
    p = predictors[torch.float16]
    boxes = torch.as_tensor(gold["boxes_in"], dtype=torch.float, device=dev)
    for multi in (False, True):
        together = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=multi, return_logits=True)
        assert together[0].shape == (3, 3 if multi else 1, 96, 128)
        for i in range(3):
            alone = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes[i:i + 1], multimask_output=multi, return_logits=True)
            for name, a, t in zip(("masks", "iou", "low"), alone, together):
                assert torch.equal(a, t[i:i + 1]), f"box {i}, multimask {multi}: {name} differs alone and in a batch of 3"
    # multimask_output=True is masks 1..3 and False mask 0 of the same four: against all four hypernetwork rows through the same kernels
    m = p.model
    sparse, dense = m.prompt_encoder(points=None, boxes=boxes[:1], masks=None)
    pe = m.prompt_encoder.get_dense_pe()
    one = m.mask_decoder.forward_features(p.features, pe, sparse, dense, False)
    three = m.mask_decoder.forward_features(p.features, pe, sparse, dense, True)
    assert one["masks"].shape == (1, 1, 256, 256) and three["masks"].shape == (1, 3, 256, 256) and one["iou"].shape == (1, 1) and three["iou"].shape == (1, 3)
    md = m.mask_decoder
    hyper = torch.stack([md._mlp(one["final_queries"][:, 1 + k:2 + k, :], md.output_hypernetworks_mlps[k])[:, 0] for k in range(4)], dim=1).contiguous()
    four = ops.sam_mask_logits(hyper, one["upscaled"])
    assert torch.equal(four[:, 0:1], one["masks"]) and torch.equal(four[:, 1:4], three["masks"])
    assert not torch.equal(one["masks"][:, 0], three["masks"][:, 0])


def test_full_width_l0_smoke(dev):
    """efficientvit_sam("l0") with seeded weights on a 1024 x 1024 image and one box: predict's returns have the reference's shapes and dtypes."""
    model = sam.efficientvit_sam("l0", device=dev)
    with torch.no_grad():
        seed_encoder(model.image_encoder, 3)
    pe, md = st.build()
    sd = {"prompt_encoder." + k: v for k, v in st.seed_state(pe, 1).state_dict().items()}
    sd.update({"mask_decoder." + k: v for k, v in st.seed_state(md, 2).state_dict().items()})
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("image_encoder.") for k in missing)
    p = sam.EfficientViTSamPredictor(model)
    image = np.random.RandomState(0).randint(0, 256, (1024, 1024, 3)).astype(np.uint8)
    p.set_image(image)
    assert p.features.shape == (1, 64, 64, 256) and p.input_size == (1024, 1024)
    masks, iou, low = p.predict(box=np.array([100.0, 150.0, 800.0, 900.0]), multimask_output=False)
    assert masks.dtype == np.bool_ and masks.shape == (1, 1024, 1024)
    assert iou.shape == (1,) and iou.dtype == np.float32
    assert low.shape == (1, 256, 256) and low.dtype == np.float32
    assert np.isfinite(low).all() and np.isfinite(iou).all()
    logits = p.predict(box=np.array([100.0, 150.0, 800.0, 900.0]), multimask_output=False, return_logits=True)[0]
    assert logits.dtype == np.float32 and np.isfinite(logits).all() and np.array_equal(logits > 0, masks)


# ------------------------------------------------------------------------------------------------ a second checkpoint into a live model
class _Parent(torch.nn.Module):
    def __init__(self, child):
        super().__init__()
        self.child = child


def _seeded_checkpoint(cfg, seed):
    """A checkpoint-shaped fp32 state dict of the narrow xl model (tests/test_effvit_xl.py::narrow_sam), seeded."""
    from omg_amd.efficientvit import EfficientViTSamImageEncoder
    enc = EfficientViTSamImageEncoder(cfg, dtype=torch.float32, device="cpu")
    seed_encoder(enc, seed)
    pe, md = st.build((64, 64), (128, 128), mlp_dim=128)
    sd = {"child.image_encoder." + k: v.clone() for k, v in enc.state_dict().items()}
    sd.update({"child.prompt_encoder." + k: v for k, v in st.seed_state(pe, seed + 1).state_dict().items()})
    sd.update({"child.mask_decoder." + k: v for k, v in st.seed_state(md, seed + 2).state_dict().items()})
    return sd


def test_a_second_checkpoint_loaded_through_a_parent_replaces_every_derived_operand(dev):
    """Load A through a parent module, run, load B through the parent, run again: masks, IoU predictions and the dense positional encoding
    are the bits of a model that only ever saw B — the same kernels on the same operands.  ``nn.Module.load_state_dict`` on a parent
    calls no child's ``load_state_dict``; packed weights kept from A (BatchNorm folds of the encoder, the decoder's transposed-convolution
    operands, the positional encoding of A's Gaussian matrix) would show here."""
    from tests.effvit_xl_torch import load_fixture_xl
    from tests.test_effvit_xl import narrow_sam
    cfg = load_fixture_xl()[1]
    sd_a, sd_b = _seeded_checkpoint(cfg, 11), _seeded_checkpoint(cfg, 23)
    image = np.random.RandomState(5).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    box = torch.tensor([[20.0, 10.0, 100.0, 80.0]], device=dev)

    def run(model):
        p = sam.EfficientViTSamPredictor(model)
        p.set_image(image)
        masks, iou, _ = p.predict_torch(point_coords=None, point_labels=None, boxes=box, multimask_output=False, return_logits=True)
        return masks, iou, model.prompt_encoder.get_dense_pe()

    live = _Parent(narrow_sam(cfg, torch.float16).to(dev))
    live.load_state_dict(sd_a, strict=True)
    first = run(live.child)
    live.load_state_dict(sd_b, strict=True)
    second = run(live.child)
    fresh = _Parent(narrow_sam(cfg, torch.float16).to(dev))
    fresh.load_state_dict(sd_b, strict=True)
    want = run(fresh.child)
    assert all(torch.isfinite(t.float()).all() for t in want)
    for name, a, w in zip(("masks", "iou", "dense_pe"), first, want):
        assert not torch.equal(a, w), f"{name}: checkpoints A and B do not tell apart"
    for name, g, w in zip(("masks", "iou", "dense_pe"), second, want):
        assert torch.equal(g, w), f"{name} after the reload differs from a model that only saw B"
