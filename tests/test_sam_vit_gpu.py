"""SAM's ViT image encoder on the GPU (-m gpu): omg_attn_relpos and omg_gelu_erf (csrc/sam_vit.hip) against torch fp32 on the same
16-bit operands, then omg_amd.sam_vit / omg_amd.segment_anything against the fixture of tests/golden/make_golden_sam_vit.py.

Tolerances are tests/test_sam_gpu.py's: for a kernel, the same computation is done by torch on the GPU in the storage dtype, its error
E against the fp32 result is measured, and the HIP kernel is allowed 2 E plus one ulp of the storage dtype at the output's largest
magnitude (``check``); for the narrow models, max |d| / rms of the golden tensor below BASE sqrt(depth) (``stage``); masks by the
``masks_agree`` rule.  Cases with an exact answer are compared bitwise.  With OMG_SAM_VIT_ERRORS_JSON=path the measured values are
written there when the module is done.

The fp32 reference of the attention is built literally: F.pad, the window partition, the einsum bias on the unscaled q, softmax.
Operands are drawn on the bf16 grid, which fp16 holds exactly at these magnitudes, so one reference serves both storage dtypes."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from omg_amd import ops, segment_anything as sa
from tests import sam_torch as st
from tests import sam_vit_torch as vt
from tests import test_sam_gpu as tg

DTYPES = [torch.float16, torch.bfloat16]
BASE = tg.BASE
MEASURED = {}
CANARY = 1234.0
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_vit_golden.npz")
GLOBAL_GRIDS = [(1, 1), (5, 7), (16, 16), (64, 64)]
# window 14: no padding; windows that are mostly padding; partial windows in both axes; SAM's grid; and a small odd window
WINDOWED = [(14, (14, 14)), (14, (16, 16)), (14, (30, 17)), (14, (64, 64)), (3, (7, 5))]


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("OMG_SAM_VIT_ERRORS_JSON")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def name(dtype):
    return str(dtype)[6:]


def check(tag, dtype, got, ref32, torch16):
    """tests/test_sam_gpu.py's ``check`` into this module's record."""
    e_torch = (torch16.float().cpu() - ref32).abs().max().item()
    e_hip = (got.float().cpu() - ref32).abs().max().item()
    bound = 2.0 * e_torch + tg.ulp(dtype, ref32.abs().max().item())
    MEASURED[tag] = {"torch_storage_dtype_err": e_torch, "hip_err": e_hip, "bound": bound, "max_abs_ref": ref32.abs().max().item()}
    print(f"{tag}: hip {e_hip:.3e}  torch-{name(dtype)} {e_torch:.3e}  bound {bound:.3e}")
    assert math.isfinite(e_hip) and e_hip <= bound, (tag, e_hip, bound)


# ------------------------------------------------------------------------------------------------ the literal reference
def relpos_ref(q, k, v, Rh, Rw, S, kpad, vpad, scale):
    """q, k, v [B, H, W, heads, d]; Rh / Rw [2 Sh - 1, d] / [2 Sw - 1, d]; S = 0 (global) or the window; kpad / vpad [heads, d]: what a
    padded position holds.  -> [B, H, W, heads, d], in the dtype and on the device of the operands."""
    B, H, W, nh, d = q.shape
    if S:
        ph, pw = (S - H % S) % S, (S - W % S) % S
        pad = lambda x: F.pad(x, (0, 0, 0, 0, 0, pw, 0, ph))
        outside = 1 - pad(torch.ones(1, H, W, 1, 1, dtype=q.dtype, device=q.device))
        q, k, v = pad(q), pad(k) + outside * kpad, pad(v) + outside * vpad
        Hp, Wp = H + ph, W + pw
        part = lambda x: x.view(B, Hp // S, S, Wp // S, S, nh, d).permute(0, 1, 3, 2, 4, 5, 6).reshape(-1, S, S, nh, d)
        q, k, v = part(q), part(k), part(v)
        KH = KW = S
    else:
        KH, KW = H, W
    N = q.shape[0]
    iy, ix = torch.arange(KH, device=q.device), torch.arange(KW, device=q.device)
    s = torch.einsum("nyxhd,nYXhd->nhyxYX", q, k) * scale
    s += torch.einsum("nyxhd,yYd->nhyxY", q, Rh[iy[:, None] - iy[None, :] + KH - 1])[..., :, None]
    s += torch.einsum("nyxhd,xXd->nhyxX", q, Rw[ix[:, None] - ix[None, :] + KW - 1])[..., None, :]
    p = torch.softmax(s.reshape(N, nh, KH, KW, KH * KW), dim=-1)
    del s
    o = torch.einsum("nhyxK,nKhd->nyxhd", p, v.reshape(N, KH * KW, nh, d))
    if S:
        o = o.reshape(B, Hp // S, Wp // S, S, S, nh, d).permute(0, 1, 3, 2, 4, 5, 6).reshape(B, Hp, Wp, nh, d)[:, :H, :W]
    return o


def bf16_grid(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16().float()


@functools.lru_cache(maxsize=16)
def case(d, heads, B, H, W, S):
    """Operands (fp32 values on the bf16 grid) and the fp32 references with a non-zero and with a null pad row; computed once, shared by
    the storage dtypes, never modified."""
    KH, KW = (S, S) if S else (H, W)
    q, k, v = (bf16_grid(B, H, W, heads, d, seed=s) for s in (1, 2, 3))
    Rh, Rw = bf16_grid(2 * KH - 1, d, seed=4, scale=d ** -0.5), bf16_grid(2 * KW - 1, d, seed=5, scale=d ** -0.5)
    kpad, vpad = bf16_grid(heads, d, seed=6), bf16_grid(heads, d, seed=7, scale=2.0)
    scale = d ** -0.5
    ref = relpos_ref(q, k, v, Rh, Rw, S, kpad, vpad, scale)
    ref0 = relpos_ref(q, k, v, Rh, Rw, S, 0 * kpad, 0 * vpad, scale) if S else None
    return dict(q=q, k=k, v=v, Rh=Rh, Rw=Rw, kpad=kpad, vpad=vpad, scale=scale, ref=ref, ref0=ref0)


def run_relpos(q, k, v, Rh, Rw, S, kpad, vpad, scale, dtype, dev):
    """The kernel on a strided column slice of a wider buffer (q | k | v head-major, as Linear(D, 3D) writes them) into a canary frame."""
    B, H, W, nh, d = q.shape
    M, hd = B * H * W, nh * d
    wide = torch.full((M, 3 * hd + 24), 7.0, dtype=dtype)
    wide[:, 8:8 + 3 * hd] = torch.cat([t.reshape(M, hd) for t in (q, k, v)], dim=1).to(dtype)
    qkv = wide.to(dev)[:, 8:8 + 3 * hd]
    frame = torch.full((M + 1, hd + 16), CANARY, dtype=dtype, device=dev)
    out = frame[:M, 8:8 + hd]
    pad = torch.cat([kpad.reshape(-1), vpad.reshape(-1)]).to(dtype).to(dev) if kpad is not None else None
    got = ops.attn_relpos(qkv, B, H, W, nh, Rh.to(dtype).to(dev), Rw.to(dtype).to(dev), scale, window=S, pad_kv=pad, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.all(frame[:, :8] == CANARY) and torch.all(frame[:, 8 + hd:] == CANARY) and torch.all(frame[M] == CANARY), "wrote outside the row"
    return got.reshape(B, H, W, nh, d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("d", [64, 80])
def test_attn_relpos_global(dev, dtype, d, heads, B):
    """One key, an odd grid (35 keys: a partial tile), 256 keys (four tiles, two query blocks), SAM's 64 x 64 (the one-row-per-tile form)."""
    for (H, W) in GLOBAL_GRIDS:
        c = case(d, heads, B, H, W, 0)
        dv = lambda t: t.to(dtype).to(dev)
        t16 = relpos_ref(dv(c["q"]), dv(c["k"]), dv(c["v"]), dv(c["Rh"]), dv(c["Rw"]), 0, None, None, c["scale"])
        got = run_relpos(c["q"], c["k"], c["v"], c["Rh"], c["Rw"], 0, None, None, c["scale"], dtype, dev)
        check(f"attn_relpos global {name(dtype)} d{d} h{heads} B{B} {H}x{W}", dtype, got, c["ref"], t16)
        del t16


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("d", [64, 80])
def test_attn_relpos_windowed(dev, dtype, d, heads, B):
    """Every window case with a non-zero pad row and with a null one (zeros)."""
    for S, (H, W) in WINDOWED:
        c = case(d, heads, B, H, W, S)
        dv = lambda t: t.to(dtype).to(dev)
        for tag, kp, vp, ref in (("pad", c["kpad"], c["vpad"], c["ref"]), ("null", None, None, c["ref0"])):
            zk = dv(c["kpad"]) if kp is not None else dv(0 * c["kpad"])
            zv = dv(c["vpad"]) if vp is not None else dv(0 * c["vpad"])
            t16 = relpos_ref(dv(c["q"]), dv(c["k"]), dv(c["v"]), dv(c["Rh"]), dv(c["Rw"]), S, zk, zv, c["scale"])
            got = run_relpos(c["q"], c["k"], c["v"], c["Rh"], c["Rw"], S, kp, vp, c["scale"], dtype, dev)
            check(f"attn_relpos window {S} {name(dtype)} d{d} h{heads} B{B} {H}x{W} {tag}", dtype, got, ref, t16)


# ------------------------------------------------------------------------------------------------ exact answers
def ints(*shape, seed, lo=1, hi=8):
    """Non-zero small integers: +-lo .. +-hi."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 80])
def test_uniform_mean_includes_padded_positions(dev, dtype, d):
    """q = 0 and zero tables: every score is 0, the result is the mean of v over the window's 64 positions INCLUDING the padded ones
    (which hold v_pad) — sums of small integers over a power of two: exact.  Window 8 on a 12 x 12 grid: one full window, two
    half-padded, one three-quarters padded.  And the global 16 x 16 mean over 256 keys."""
    B, heads, S, H, W = 2, 2, 8, 12, 12
    q = torch.zeros(B, H, W, heads, d)
    k = bf16_grid(B, H, W, heads, d, seed=12)
    v = ints(B, H, W, heads, d, seed=11)
    vpad = ints(heads, d, seed=13)
    kpad = bf16_grid(heads, d, seed=14)
    Rz = torch.zeros(2 * S - 1, d)
    for kp, vp in ((kpad, vpad), (None, None)):
        want = relpos_ref(q, k, v, Rz, Rz, S, 0 * kpad if kp is None else kp, 0 * vpad if vp is None else vp, d ** -0.5)
        full = v[:, :8, :8].mean(dim=(1, 2))                                              # the unpadded window: the plain mean
        assert torch.equal(want[:, 0, 0], full) and not torch.equal(want[:, 11, 11], want[:, 0, 0])
        got = run_relpos(q, k, v, Rz, Rz, S, kp, vp, d ** -0.5, dtype, dev)
        assert torch.equal(got.float().cpu(), want.to(dtype).float())
    Rz = torch.zeros(31, d)
    v = ints(B, 16, 16, heads, d, seed=15)
    want = v.mean(dim=(1, 2), keepdim=True).expand(B, 16, 16, heads, d)
    got = run_relpos(torch.zeros(B, 16, 16, heads, d), bf16_grid(B, 16, 16, heads, d, seed=16), v, Rz, Rz, 0, None, None, d ** -0.5, dtype, dev)
    assert torch.equal(got.float().cpu(), want.to(dtype).float())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 80])
@pytest.mark.parametrize("off", [(2, -1), (-3, 2)])
@pytest.mark.parametrize("S,H,W", [(0, 9, 11), (0, 64, 64), (14, 16, 16)])
def test_one_hot_bias_selects_the_key_at_the_offset(dev, dtype, d, off, S, H, W):
    """k = 0, q = e_0, Rh[dy0 + Sh - 1] = Rw[dx0 + Sw - 1] = 40 e_0 and zero elsewhere: the key at (qy - dy0, qx - dx0) scores 80, a key
    sharing one coordinate 40, the rest 0.  exp(-40) is below half an ulp of a non-zero integer v, so the output of a query whose target
    is inside its grid / window is that key's v (or v_pad) bit for bit.  Different offsets in the two axes and both signs: a swapped
    axis or a flipped sign selects another key."""
    dy0, dx0 = off
    B, heads = 1, 2
    KH, KW = (S, S) if S else (H, W)
    q = torch.zeros(B, H, W, heads, d)
    q[..., 0] = 1.0
    k = torch.zeros(B, H, W, heads, d)
    v = ints(B, H, W, heads, d, seed=21)
    vpad = ints(heads, d, seed=22)
    Rh, Rw = torch.zeros(2 * KH - 1, d), torch.zeros(2 * KW - 1, d)
    Rh[dy0 + KH - 1, 0] = 40.0
    Rw[dx0 + KW - 1, 0] = 40.0
    got = run_relpos(q, k, v, Rh, Rw, S, torch.zeros(heads, d) if S else None, vpad if S else None, d ** -0.5, dtype, dev).float().cpu()
    n = 0
    for y in range(H):
        for x in range(W):
            oy, ox = (y // S * S, x // S * S) if S else (0, 0)
            ty, tx = y - dy0, x - dx0
            if not (oy <= ty < oy + KH and ox <= tx < ox + KW):
                continue                                                                  # the target is outside the window: no key scores 80
            want = v[0, ty, tx] if (ty < H and tx < W) else vpad
            assert torch.equal(got[0, y, x], want), (y, x)
            n += 1
    assert n >= (KH - 3) * (KW - 2) or S


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 80])
def test_dominant_padded_key(dev, dtype, d):
    """k = 0 for real tokens and k_pad = 512 e_0 against q = e_0: a padded key scores 512 scale >= 57, a real one 0.  Queries of the three
    border windows return v_pad; the interior window has no padded key and returns the plain mean."""
    B, heads, S, H, W = 1, 2, 8, 12, 12
    q = torch.zeros(B, H, W, heads, d)
    q[..., 0] = 1.0
    k = torch.zeros(B, H, W, heads, d)
    v = ints(B, H, W, heads, d, seed=31)
    vpad = ints(heads, d, seed=32)
    kpad = torch.zeros(heads, d)
    kpad[:, 0] = 512.0
    Rz = torch.zeros(2 * S - 1, d)
    got = run_relpos(q, k, v, Rz, Rz, S, kpad, vpad, d ** -0.5, dtype, dev).float().cpu()
    border = torch.ones(H, W, dtype=torch.bool)
    border[:8, :8] = False
    assert torch.equal(got[0][border], vpad.expand(int(border.sum()), heads, d))
    assert torch.equal(got[0, :8, :8], v[0, :8, :8].mean(dim=(0, 1), keepdim=True).expand(8, 8, heads, d).to(dtype).float())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 80])
@pytest.mark.parametrize("H,W", [(16, 16), (64, 64)])
def test_running_maximum_at_huge_scores(dev, dtype, d, H, W):
    """q . k = +-60000 (240 * 250), as test_attn_small_running_maximum_at_huge_scores: exp overflows without the running maximum, and
    the maximum moves late, at the last four keys.  The answer is exactly the mean of their four rows of V."""
    B, heads = 1, 2
    q = torch.zeros(B, H, W, heads, d)
    q[..., 0] = 240.0
    k = torch.zeros(B, H * W, heads, d)
    k[..., 0] = -250.0
    k[:, -4:, :, 0] = 250.0
    v = ints(B, H * W, heads, d, seed=41)
    want = v[:, -4:].mean(dim=1)[:, None, None].expand(B, H, W, heads, d)
    assert torch.equal(want, want.to(dtype).float())
    Rz_h, Rz_w = torch.zeros(2 * H - 1, d), torch.zeros(2 * W - 1, d)
    got = run_relpos(q, k.view(B, H, W, heads, d), v.view(B, H, W, heads, d), Rz_h, Rz_w, 0, None, None, d ** -0.5, dtype, dev)
    assert torch.equal(got.float().cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 80])
def test_a_samples_rows_do_not_depend_on_the_batch(dev, dtype, d):
    heads = 3
    for S, (H, W) in [(0, (16, 16)), (14, (30, 17))]:
        c = case(d, heads, 2, H, W, S)
        kp, vp = (c["kpad"], c["vpad"]) if S else (None, None)
        both = run_relpos(c["q"], c["k"], c["v"], c["Rh"], c["Rw"], S, kp, vp, c["scale"], dtype, dev)
        for b in range(2):
            alone = run_relpos(c["q"][b:b + 1], c["k"][b:b + 1], c["v"][b:b + 1], c["Rh"], c["Rw"], S, kp, vp, c["scale"], dtype, dev)
            assert torch.equal(alone[0], both[b]), (S, H, W, b)


# ------------------------------------------------------------------------------------------------ omg_gelu_erf
@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_erf(dev, dtype):
    for shape in [(3, 7, 2048), (37, 8)]:                                                  # 296 elements: not a multiple of 256
        x = (torch.randn(*shape, generator=torch.Generator().manual_seed(61)) * 3).to(dtype)
        ref32 = F.gelu(x.float())
        xd = x.to(dev)
        t16 = F.gelu(xd)
        got = ops.gelu_erf(xd)
        check(f"gelu_erf {name(dtype)} {shape}", dtype, got, ref32, t16)
        y = xd.clone()
        assert ops.gelu_erf(y, out=y).data_ptr() == y.data_ptr() and torch.equal(y, got)


# ================================================================================================ the modules and the predictor
# Per stage, tests/test_sam_gpu.py's convention: max |d| / rms of the golden tensor below BASE sqrt(depth), depth = blocks in front of
# the tensor: 1 for the patch embedding, 2 per transformer block (attention, MLP), 2 for the neck; the decoder's stages on top of the
# encoder's as there.  The mask comparison runs in fp16, the predictor's default; bf16 is compared per stage.
MODELS = ["d64", "d80"]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def predictors(dev, gold):
    """(model, dtype) -> a predictor of the narrow model with the fixture's image_a set (built once, never modified by a test)."""
    out = {}
    for m in MODELS:
        for dt in DTYPES:
            p = sa.SamPredictor(vt.narrow_model(gold, m, dt, dev))
            p.set_image(gold["image_a"])
            out[(m, dt)] = p
    return out


def stage(tag, dtype, got, ref, depth, failed):
    got, ref = got.float().cpu(), torch.as_tensor(ref).float()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    rel = (got - ref).abs().max().item() / ref.pow(2).mean().sqrt().item()
    bound = BASE[dtype] * math.sqrt(depth)
    MEASURED[f"{name(dtype)} {tag}"] = {"rel_err_max_over_rms": rel, "depth": depth, "bound": bound}
    print(f"narrow sam {name(dtype)} {tag}: max |d| / rms {rel:.3e}  (depth {depth}, bound {bound:.3e})")
    if not (math.isfinite(rel) and rel < bound):
        failed.append((tag, rel, bound))


def at(t, idx):
    i = torch.as_tensor(idx, device=t.device)
    return t[:, i][:, :, i]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_narrow_model_matches_the_reference_per_stage(dev, model, dtype, gold, predictors):
    p = predictors[(model, dtype)]
    m = p.model
    P = model + "."
    assert p.input_size == (768, 1024) and p.original_size == (48, 64) and p.is_image_set
    emb = p.get_image_embedding()
    assert emb.shape == (1, 256, 64, 64) and emb.dtype == dtype and emb.data_ptr() == p.features.data_ptr()
    idx, subl = gold["cfg_idx"].tolist(), int(gold["cfg_sub_low"])
    resized = vt.resize_longest(gold["image_a"])
    assert np.allclose(st.checksum(torch.from_numpy(resized.astype(np.float64))), gold["resized_a_sum"], rtol=1e-12, atol=0)
    x = m.preprocess(torch.from_numpy(resized).permute(2, 0, 1)[None].to(dev)).to(dtype)
    f = m.image_encoder.forward_features(x)
    assert torch.equal(f["out"], p._features_nhwc)
    depth = len(m.image_encoder.blocks)
    failed = []
    stage(f"{model} patch_embed", dtype, at(f["patch_embed"], idx), gold[P + "patch_embed"], 1, failed)
    for i in range(depth):
        stage(f"{model} block{i}", dtype, at(f[f"block{i}"], idx), gold[P + f"block{i}"], 1 + 2 * (i + 1), failed)
    d0 = 1 + 2 * depth + 2
    stage(f"{model} features", dtype, at(f["out"], idx).permute(0, 3, 1, 2), gold[P + "features"], d0, failed)
    boxes = torch.as_tensor(gold["boxes_in"], dtype=torch.float, device=dev)
    assert torch.allclose(p.transform.apply_boxes_torch(torch.as_tensor(gold["boxes"], device=dev), p.original_size), boxes, rtol=1e-6)
    masks, iou, low = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)
    assert masks.dtype == torch.bool and masks.shape == (3, 1, 48, 64) and iou.shape == (3, 1) and low.shape == (3, 1, 256, 256) and low.dtype == torch.float32
    stage(f"{model} low-resolution logits", dtype, low[:, :, ::subl, ::subl], gold[P + "low_boxes"], d0 + 13, failed)
    stage(f"{model} iou", dtype, iou, gold[P + "iou_boxes"], d0 + 10, failed)
    mp, ip, lp = p.predict(point_coords=gold["points"], point_labels=gold["point_labels"], multimask_output=True)
    assert mp.shape == (3, 48, 64) and mp.dtype == np.bool_ and ip.shape == (3,) and lp.shape == (3, 256, 256) and lp.dtype == np.float32
    stage(f"{model} predict(points) low-resolution logits", dtype, torch.from_numpy(lp[None, :, ::subl, ::subl]), gold[P + "low_points"], d0 + 13, failed)
    stage(f"{model} predict(points) iou", dtype, torch.from_numpy(ip[None]), gold[P + "iou_points"], d0 + 10, failed)
    assert not failed, failed


def masks_agree(tag, got_masks, gold_masks, gold_logits, err, mult):
    sel = np.abs(gold_logits) > mult * err
    excluded = 1.0 - sel.mean()
    wrong = int((got_masks[sel] != gold_masks[sel]).sum())
    MEASURED[f"float16 masks {tag}"] = {"low_res_logit_err": err, "excluded_share": excluded, "wrong_pixels": wrong, "area": float(gold_masks.mean())}
    print(f"masks {tag}: low-resolution logit error {err:.3e}, excluded share {excluded:.4f}, wrong among the rest {wrong}, golden area {gold_masks.mean():.3f}")
    assert wrong == 0 and excluded <= 0.02, (tag, wrong, excluded)


@pytest.mark.parametrize("model", MODELS)
def test_final_masks_match_the_reference(dev, model, gold, predictors):
    p = predictors[(model, torch.float16)]
    P = model + "."
    mult, subl = float(gold["cfg_mask_mult"]), int(gold["cfg_sub_low"])
    boxes = torch.as_tensor(gold["boxes_in"], dtype=torch.float, device=dev)
    masks, iou, low = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)
    err = float((low[:, :, ::subl, ::subl].cpu() - torch.from_numpy(gold[P + "low_boxes"])).abs().max())
    masks_agree(f"{model} 3 boxes", masks.cpu().numpy(), gold[P + "masks_boxes"], gold[P + "logits_boxes"], err, mult)
    logits = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False, return_logits=True)[0]
    assert logits.dtype == torch.float32 and torch.equal(logits > 0, masks)
    m1, i1, l1 = p.predict(box=gold["boxes"][0], multimask_output=False)
    assert m1.dtype == np.bool_ and m1.shape == (1, 48, 64) and i1.shape == (1,) and l1.shape == (1, 256, 256)
    assert np.array_equal(m1, masks[0].cpu().numpy())
    mp, _, lp = p.predict(point_coords=gold["points"], point_labels=gold["point_labels"], multimask_output=True)
    err_p = float(np.abs(lp[None, :, ::subl, ::subl] - gold[P + "low_points"]).max())
    masks_agree(f"{model} predict(points)", mp[None], gold[P + "masks_points"], gold[P + "logits_points"], err_p, mult)
    # the second image: no host resize, another input_size
    q = sa.SamPredictor(p.model)
    q.set_image(gold["image_b"])
    assert q.input_size == (16, 1024) and q.original_size == (16, 1024)
    mb, _, lb = q.predict(box=gold["box_b"], multimask_output=False)
    err_b = float(np.abs(lb[None, :, ::subl, ::subl] - gold[P + "low_b"]).max())
    masks_agree(f"{model} image_b", mb[None], gold[P + "masks_b"], gold[P + "logits_b"], err_b, mult)


def test_set_torch_image_equals_set_image_and_boxes_do_not_depend_on_the_batch(dev, gold, predictors):
    p = predictors[("d80", torch.float16)]
    q = sa.SamPredictor(p.model)
    resized = torch.from_numpy(vt.resize_longest(gold["image_a"])).permute(2, 0, 1)[None].to(dev)
    q.set_torch_image(resized, gold["image_a"].shape[:2])
    assert q.input_size == p.input_size and q.original_size == p.original_size and torch.equal(q.features, p.features)
    q.set_image(gold["image_a"][..., ::-1], image_format="BGR")
    assert torch.equal(q.features, p.features)
    q.reset_image()
    assert not q.is_image_set and q.features is None
    boxes = torch.as_tensor(gold["boxes_in"], dtype=torch.float, device=dev)
    for multi in (False, True):
        together = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=multi, return_logits=True)
        assert together[0].shape == (3, 3 if multi else 1, 48, 64)
        for i in range(3):
            alone = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes[i:i + 1], multimask_output=multi, return_logits=True)
            for what, a, t in zip(("masks", "iou", "low"), alone, together):
                assert torch.equal(a, t[i:i + 1]), f"box {i}, multimask {multi}: {what} differs alone and in a batch of 3"


# ------------------------------------------------------------------------------------------------ full width
def full_width_smoke(build, dev):
    model = build(device=dev)
    rs = np.random.RandomState(5)
    with torch.no_grad():
        for key, t in model.state_dict().items():
            if not t.dtype.is_floating_point:
                continue
            z = torch.from_numpy(rs.standard_normal(tuple(t.shape)).astype(np.float32))
            if key.endswith("pos_embed"):
                v = 0.5 * z
            elif "norm" in key or ".neck.1." in key or ".neck.3." in key or "output_upscaling.1." in key or "mask_downscaling.1." in key or "mask_downscaling.4." in key:
                v = 1.0 + 0.2 * z if key.endswith("weight") else 0.1 * z
            elif key.endswith("bias"):
                v = 0.1 * z
            elif t.dim() < 2 or "gaussian_matrix" in key or "embed" in key or "token" in key:
                v = z
            elif "output_upscaling" in key:
                v = z / math.sqrt(t.shape[0])
            else:
                v = z / math.sqrt(t[0].numel())
            t.copy_(v.to(t.dtype))
    p = sa.SamPredictor(model)
    image = np.random.RandomState(0).randint(0, 256, (1024, 1024, 3)).astype(np.uint8)
    p.set_image(image)
    assert p.get_image_embedding().shape == (1, 256, 64, 64) and p.input_size == (1024, 1024)
    assert torch.isfinite(p.features.float()).all()
    boxes = p.transform.apply_boxes_torch(torch.tensor([[100.0, 150.0, 800.0, 900.0]], device=dev), image.shape[:2])
    masks, iou, low = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)
    assert masks.dtype == torch.bool and masks.shape == (1, 1, 1024, 1024) and iou.shape == (1, 1) and low.shape == (1, 1, 256, 256)
    assert torch.isfinite(low).all() and torch.isfinite(iou).all()
    area = masks.float().mean().item()
    print(f"full width: mask area {area:.3f}")
    assert 0.0 < area < 1.0, "the mask is empty or full"


def test_full_width_vit_b_smoke(dev):
    full_width_smoke(sa.build_sam_vit_b, dev)


@pytest.mark.slow
def test_full_width_vit_h_smoke(dev):
    full_width_smoke(sa.build_sam_vit_h, dev)
