"""The xl EfficientViT-SAM path on the HIP kernels (-m gpu): omg_litemla_aggreg against torch fp32 on the same 16-bit operands, LiteMLA
with the fused aggregation against the GEMM one, the narrow six-stage encoder and predictor against the fixtures of the reference's own
classes (tests/golden/effvit_xl_golden.npz, sam_xl_golden.npz), batch invariance, and the full-width xl0 against a per-layer fallback.

The kernel's tolerance is measured as in tests/test_effvit_gpu.py (its ``check``): torch does the same computation on the GPU in the
storage dtype, rounding between the two convolutions as the kernel does; its error E against fp32 is taken, and the kernel is allowed
2 E plus one ulp.  With OMG_EFFVIT_ERRORS_JSON=path the measured values are written there when the module is done."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from omg_amd import ops, sam
from omg_amd.efficientvit import EfficientViTSamConfig, EfficientViTSamImageEncoder
from omg_amd.litemla import LiteMLA
from oracle import litemla as ol
from tests.effvit_torch import TorchEncoder, seed_encoder
from tests.effvit_xl_torch import GOLD_SAM, build_xl, load_fixture_xl, narrow_sam_xl
from tests.test_effvit_gpu import BASE, CANARY, DTYPES, MEASURED, SIZES, check, nhwc, rnd


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("OMG_EFFVIT_ERRORS_JSON")
    if path and MEASURED:                                             # the sibling's dict: what it measured in this session stays in the file
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def fixture():
    return load_fixture_xl()


def name(dtype):
    return str(dtype)[6:]


# ------------------------------------------------------------------------------------------------ the kernel
def aggreg_operands(B, H, W, C, s, dim, dtype, seed):
    x = rnd(B, C, H, W, seed=seed, dtype=dtype)
    wd = rnd(C, 1, s, s, seed=seed + 1, scale=1.0 / s, dtype=dtype)
    wg = rnd(C, dim, 1, 1, seed=seed + 2, scale=dim ** -0.5, dtype=dtype)
    return x, wd, wg


def run_aggreg(x, wd, wg, s, dim, dev, pad_value=CANARY):
    """The kernel on column slices of ONE wider buffer (input at columns 8 .., output behind it, canary columns round both and a canary
    row behind the last pixel) -> (result NCHW on the device, the buffer before, the buffer after, the output's column range)."""
    B, C, H, W = x.shape
    M, ld = B * H * W, 2 * C + 32
    buf = torch.full((M + 1, ld), pad_value, dtype=x.dtype)
    buf[:M, 8:8 + C] = nhwc(x).reshape(M, C)
    before = buf.clone()
    buf = buf.to(dev)
    lo = 16 + C
    taps = wd.reshape(C, s * s).t().contiguous().to(dev)
    out = ops.litemla_aggreg(buf[:M, 8:8 + C], taps, wg.reshape(C, dim).contiguous().to(dev), B, H, W, s, dim, out=buf[:M, lo:lo + C])
    assert out.data_ptr() == buf[:M, lo:lo + C].data_ptr()
    return out.reshape(B, H, W, C).permute(0, 3, 1, 2), before, buf.cpu(), (lo, lo + C)


def untouched(before, after, cols, M):
    keep = torch.ones_like(before, dtype=torch.bool)
    keep[:M, cols[0]:cols[1]] = False
    return torch.equal(before[keep], after[keep])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("dim", [16, 32])
def test_litemla_aggreg(dev, dtype, dim, heads):
    """heads 1 at dim 16 is 48 channels: one and a half tiles of 32; heads 3 at dim 32 is 288: nine tiles over three blocks of four
    waves.  7 x 9 has no interior pixel for s = 5 in one direction and a pixel tail in the last block; 2 x 32 x 32 is 64 pixel blocks."""
    B, C = 2, 3 * heads * dim
    with torch.backends.cudnn.flags(enabled=False):
        for (H, W) in SIZES:
            for s in (3, 5):
                x, wd, wg = aggreg_operands(B, H, W, C, s, dim, dtype, seed=20)
                mid32 = F.conv2d(x.float(), wd.float(), padding=s // 2, groups=C)
                ref32 = F.conv2d(mid32, wg.float(), groups=C // dim)
                mid16 = F.conv2d(x.to(dev), wd.to(dev), padding=s // 2, groups=C)          # rounded to the storage dtype here, as in the kernel
                t16 = F.conv2d(mid16, wg.to(dev), groups=C // dim)
                assert mid16.dtype == dtype and t16.dtype == dtype
                got, before, after, cols = run_aggreg(x, wd, wg, s, dim, dev)
                assert untouched(before, after, cols, B * H * W), "wrote outside its column slice or past the last pixel"
                check(f"litemla_aggreg {name(dtype)} dim{dim} heads{heads} s{s} {H}x{W}", dtype, got, ref32, t16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,heads,s", [(16, 1, 3), (16, 3, 5), (32, 1, 5), (32, 3, 3)])
def test_litemla_aggreg_exact_on_small_integers(dev, dtype, dim, heads, s):
    g = torch.Generator().manual_seed(23)
    B, H, W, C = 2, 7, 9, 3 * heads * dim
    x = torch.randint(-1, 2, (B, C, H, W), generator=g).float()
    wd = torch.randint(-1, 2, (C, 1, s, s), generator=g).float() * (torch.rand(C, 1, s, s, generator=g) < 0.5)
    wg = torch.randint(-1, 2, (C, dim, 1, 1), generator=g).float() * (torch.rand(C, dim, 1, 1, generator=g) < 0.25)
    mid = F.conv2d(x, wd, padding=s // 2, groups=C)
    ref = F.conv2d(mid, wg, groups=C // dim)
    assert torch.equal(mid, mid.to(dtype).float()) and torch.equal(ref, ref.to(dtype).float()), "the case itself must be exactly representable"
    assert mid.abs().max() >= 4 and ref.abs().max() >= 8
    got, before, after, cols = run_aggreg(x.to(dtype), wd.to(dtype), wg.to(dtype), s, dim, dev)
    assert untouched(before, after, cols, B * H * W)
    assert torch.equal(got.float().cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,s", [(16, 5), (32, 3)])
def test_litemla_aggreg_neighbours_come_from_the_same_image(dev, dtype, dim, s):
    """An image's result is bitwise the same alone and as the middle image of a batch of 3 whose other two images are full of large
    values: a tap that crossed a batch boundary would show."""
    H, W, C = 7, 9, 3 * 3 * dim
    x, wd, wg = aggreg_operands(1, H, W, C, s, dim, dtype, seed=26)
    big = torch.full_like(x, 1000.0)
    alone = run_aggreg(x, wd, wg, s, dim, dev)[0]
    three = run_aggreg(torch.cat([big, x, -big]), wd, wg, s, dim, dev)[0]
    assert torch.isfinite(alone.float()).all() and alone.float().abs().max() < 100
    assert torch.equal(three[1:2], alone)


def test_litemla_aggreg_refuses_overlapping_operands(dev):
    C, dim = 96, 32
    buf = torch.zeros((16, 2 * C), dtype=torch.float16, device=dev)
    taps, wg = torch.zeros((9, C), dtype=torch.float16, device=dev), torch.zeros((C, dim), dtype=torch.float16, device=dev)
    with pytest.raises(AssertionError, match="overlaps"):
        ops.litemla_aggreg(buf[:, :C], taps, wg, 1, 4, 4, 3, dim, out=buf[:, :C])
    with pytest.raises(AssertionError, match="overlaps"):
        ops.litemla_aggreg(buf[:, :C], taps, wg, 1, 4, 4, 3, dim, out=buf[:, 48:48 + C])
    ops.litemla_aggreg(buf[:, :C], taps, wg, 1, 4, 4, 3, dim, out=buf[:, C:])


# ------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scales", [(3,), (5,)])
@pytest.mark.parametrize("dim", [16, 32])
def test_litemla_fused_against_gemm_aggregation(dev, dtype, dim, scales):
    """The same weights through both aggregations: each within the module's bound against the fp32 oracle on the same rounded weights
    (tests/test_litemla_gpu.py::test_module_at_efficientvit_sam_shape_vs_oracle: max |d| / rms 2e-2 in fp16, 1.5e-1 in bf16)."""
    cin, B, H, W = 64, 2, 12, 10
    sd = ol.init_state_dict(cin, cin, dim, scales, seed=27, dtype=dtype)
    x = rnd(B, cin, H, W, seed=28, dtype=dtype)
    ref = ol.litemla_forward({k: v.float() for k, v in sd.items()}, x.float(), dim=dim, scales=scales) + x.float()
    rms = ref.pow(2).mean().sqrt().item()
    got = {}
    for aggreg in ("gemm", "fused"):
        m = LiteMLA(cin, cin, dim=dim, scales=scales, dtype=dtype, device=dev, aggreg=aggreg)
        res = m.load_state_dict({k: v.to(dtype) if v.dtype.is_floating_point and "running" not in k else v for k, v in sd.items()}, strict=False)
        assert all(k.endswith("num_batches_tracked") for k in res.missing_keys) and not res.unexpected_keys, res
        got[aggreg] = m(x.to(dev), residual=True).float().cpu()
        assert ("wbd" in m._packed) == (aggreg == "gemm") and ("wg" in m._packed) == (aggreg == "fused")
    bound = 2e-2 if dtype == torch.float16 else 1.5e-1
    rel = {k: (v - ref).abs().max().item() / rms for k, v in got.items()}
    between = (got["fused"] - got["gemm"]).abs().max().item() / rms
    MEASURED[f"LiteMLA {name(dtype)} dim{dim} scales{scales[0]}"] = {"gemm_vs_oracle": rel["gemm"], "fused_vs_oracle": rel["fused"], "fused_vs_gemm": between, "bound": bound}
    print(f"LiteMLA {name(dtype)} dim {dim} scales {scales}: max |d| / rms vs oracle gemm {rel['gemm']:.2e} fused {rel['fused']:.2e}; fused vs gemm {between:.2e}")
    assert rel["gemm"] < bound and rel["fused"] < bound, rel


# ------------------------------------------------------------------------------------------------ the encoder
def depths(cfg):
    """tests/test_effvit_gpu.py::depths with the xl block names: the stem, every downsample block, every ResBlock / FusedMBConv / MBConv
    one each, an att or att@3 block two (its LiteMLA and its MBConv); the neck's fusion, its middle blocks, its output convolution and
    the LayerNorm one each."""
    d, n = {}, 1
    for s, dep in enumerate(cfg.depth_list):
        n += (1 if s else 0) + dep * (2 if cfg.block_list[s].startswith("att") else 1)
        d[f"stage{s}"] = n
    d["neck_mid"] = n + 1 + cfg.head_depth
    d["neck"] = d["neck_mid"] + 1
    d["out"] = d["neck"] + 1
    return d


@pytest.mark.parametrize("dtype", DTYPES)
def test_narrow_xl_encoder_matches_the_reference_classes(dev, dtype, fixture):
    _, cfg, sd, vec, sub = fixture
    m = build_xl(cfg, sd, dtype, dev)
    assert all(x.fused_aggreg and x.scales == (3,) for x in m.modules() if isinstance(x, LiteMLA))
    feats = m.forward_features(vec["x"].to(dtype).to(dev))
    emb = m(vec["x"].to(dtype).to(dev))
    assert emb.shape == (1, 256, 64, 64) and torch.equal(emb, feats["out"].permute(0, 3, 1, 2))
    failed = []
    for k, d in depths(cfg).items():
        got = feats[k].permute(0, 3, 1, 2).float().cpu()
        if k in ("neck", "out"):
            got = got[:, :, ::sub, ::sub]
        ref = vec[k]
        assert got.shape == ref.shape and torch.isfinite(got).all(), k
        rel = (got - ref).abs().max().item() / ref.pow(2).mean().sqrt().item()
        bound = BASE[dtype] * math.sqrt(d)
        MEASURED[f"xl encoder {name(dtype)} {k}"] = {"rel_err_max_over_rms": rel, "depth": d, "bound": bound}
        print(f"narrow xl encoder {dtype} {k}: max |d| / rms {rel:.3e}  (depth {d}, bound {bound:.3e})")
        if not rel < bound:
            failed.append((k, rel, bound))
    assert not failed, failed


def test_narrow_xl_encoder_batch_invariance(dev, fixture):
    _, cfg, sd, _, _ = fixture
    m = build_xl(cfg, sd, torch.float16, dev)
    x = rnd(3, 3, 128, 128, seed=29).to(dev)
    together = m(x)
    for i in range(3):
        assert torch.equal(m(x[i:i + 1]), together[i:i + 1]), f"image {i} differs alone and in a batch of 3"


def test_full_width_xl0_against_the_per_layer_fallback(dev):
    """xl0 at its real widths on a 512 x 512 input (a quarter of the pixels of its 1024 x 1024): every channel width of the model, the
    12288-channel depthwise convolution, the K = 12288 GEMM and the T = 1024 aggregation.  Finite, [1, 256, 64, 64], and equal to the
    per-layer fallback within BASE sqrt(2 depth), as the l0 test of tests/test_effvit_gpu.py.

    The whole model runs in bf16: with seed_encoder's gains the activations of this deeper model grow to 7e2 after stage 4, 1.7e4 after
    stage 5 and 2.5e5 in the neck (fp32 on the CPU, any seed and input scale tried), past fp16's largest number, so no fp16 evaluation
    of these weights is finite, whatever computes it.  fp16 is compared where it can be: every stage up to stage 4 (its att@3 blocks,
    the T = 512 aggregation and the 4096-channel depthwise convolution included), bound BASE sqrt(2 depth of that stage)."""
    cfg = EfficientViTSamConfig.xl0()
    x32 = rnd(1, 3, 512, 512, seed=30, dtype=torch.float32).half()
    for dt, keys in ((torch.bfloat16, ["out"]), (torch.float16, ["stage0", "stage1", "stage2", "stage3", "stage4"])):
        m = EfficientViTSamImageEncoder(cfg, dtype=dt, device=dev)
        seed_encoder(m, 31)
        x = x32.to(dt).to(dev)
        feats = m.forward_features(x)
        if "out" in keys:
            got = m(x)
            assert got.shape == (1, 256, 64, 64) and got.dtype == dt and torch.isfinite(got).all()
            assert torch.equal(got, feats["out"].permute(0, 3, 1, 2))
        assert all("wbd" not in l._packed and "wg" in l._packed for l in m.modules() if isinstance(l, LiteMLA))
        with torch.backends.cudnn.flags(enabled=False):
            ref = TorchEncoder(m, rounded=True).features(x)
        dep = depths(cfg)
        for k in keys:
            g, r = feats[k].permute(0, 3, 1, 2).float(), ref[k].float()
            assert g.shape == r.shape and torch.isfinite(g).all() and torch.isfinite(r).all(), (dt, k)
            rel = (g - r).abs().max().item() / r.pow(2).mean().sqrt().item()
            bound = BASE[dt] * math.sqrt(2 * dep[k])
            MEASURED[f"encoder xl0 512 {name(dt)} {k} vs per-layer fallback"] = {"rel_err_max_over_rms": rel, "depth": dep[k], "bound": bound}
            print(f"xl0 512x512 {name(dt)} {k}: max |d| / rms vs the per-layer fallback {rel:.3e}  (depth {dep[k]}, bound {bound:.3e})")
            assert rel < bound, (dt, k, rel, bound)
        del m, feats, ref
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD_SAM)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def predictor(dev, gold):
    """The fp16 predictor of the narrow xl model with the fixture's image set (built once, never modified by a test)."""
    p = sam.EfficientViTSamPredictor(narrow_sam_xl(gold, torch.float16, dev))
    p.set_image(gold["image"])
    return p


def stage(tag, dtype, got, ref, depth, failed):
    """tests/test_sam_gpu.py::stage."""
    got, ref = got.float().cpu(), torch.as_tensor(ref).float()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    rel = (got - ref).abs().max().item() / ref.pow(2).mean().sqrt().item()
    bound = BASE[dtype] * math.sqrt(depth)
    MEASURED[f"xl sam {name(dtype)} {tag}"] = {"rel_err_max_over_rms": rel, "depth": depth, "bound": bound}
    print(f"narrow xl sam {name(dtype)} {tag}: max |d| / rms {rel:.3e}  (depth {depth}, bound {bound:.3e})")
    if not (math.isfinite(rel) and rel < bound):
        failed.append((tag, rel, bound))


def masks_agree(tag, got_masks, gold_masks, gold_logits, err, mult):
    """tests/test_sam_gpu.py::masks_agree: masks are compared where the golden logit is further from the threshold than ``mult`` x the
    measured low-resolution logit error; no wrong pixel among those, and at most 2 % left out."""
    sel = np.abs(gold_logits) > mult * err
    excluded = 1.0 - sel.mean()
    wrong = int((got_masks[sel] != gold_masks[sel]).sum())
    MEASURED[f"xl sam float16 masks {tag}"] = {"low_res_logit_err": err, "excluded_share": excluded, "wrong_pixels": wrong, "area": float(gold_masks.mean())}
    print(f"xl masks {tag}: low-resolution logit error {err:.3e}, excluded share {excluded:.4f}, wrong among the rest {wrong}, golden area {gold_masks.mean():.3f}")
    assert wrong == 0 and excluded <= 0.02, (tag, wrong, excluded)


def test_narrow_xl_predictor_matches_the_reference(dev, gold, predictor):
    p = predictor
    m = p.model
    assert m.image_size == (128, 128) and p.original_size == (60, 100) and p.input_size == (77, 128) and p.features.shape == (1, 64, 64, 256)
    assert m.mask_decoder.LN_EPS == 1e-6 and m.image_encoder.norm.eps == 1e-6
    sub, subl, mult = int(gold["cfg_sub_emb"]), int(gold["cfg_sub_low"]), float(gold["cfg_mask_mult"])
    d0 = depths(m.image_encoder.cfg)["out"]
    dt = torch.float16
    failed = []
    stage("features", dt, p.features.permute(0, 3, 1, 2)[:, :, ::sub, ::sub], gold["features"], d0, failed)
    boxes = torch.as_tensor(p.apply_boxes(gold["boxes"]), dtype=torch.float, device=dev)
    assert np.allclose(boxes.cpu().numpy(), gold["boxes_in"], rtol=0, atol=1e-4)
    masks, iou, low = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)
    assert masks.dtype == torch.bool and masks.shape == (3, 1, 60, 100) and iou.shape == (3, 1) and low.shape == (3, 1, 256, 256)
    stage("low-resolution logits", dt, low[:, :, ::subl, ::subl], gold["low_boxes"], d0 + 13, failed)
    stage("iou", dt, iou, gold["iou_boxes"], d0 + 10, failed)
    assert not failed, failed
    err = float((low[:, :, ::subl, ::subl].cpu() - torch.from_numpy(gold["low_boxes"])).abs().max())
    masks_agree("3 boxes", masks.cpu().numpy(), gold["masks_boxes"], gold["logits_boxes"], err, mult)
    logits = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False, return_logits=True)[0]
    assert logits.dtype == torch.float32 and torch.equal(logits > 0, masks)
    e_final = float((logits.cpu() - torch.from_numpy(gold["logits_boxes"])).abs().max())
    print(f"xl final logits: max |d| {e_final:.3e} (low-resolution {err:.3e})")
    assert e_final <= mult * err
    m1, i1, l1 = p.predict(box=gold["boxes"][0], multimask_output=False)
    assert m1.dtype == np.bool_ and m1.shape == (1, 60, 100) and i1.shape == (1,) and l1.shape == (1, 256, 256) and l1.dtype == np.float32
    assert np.array_equal(m1, masks[0].cpu().numpy())
    masks_agree("predict(box)", m1, gold["masks_box_predict"], gold["logits_boxes"][0], err, mult)


def test_narrow_xl_predictor_batch_invariance(dev, gold, predictor):
    p = predictor
    boxes = torch.as_tensor(gold["boxes_in"], dtype=torch.float, device=dev)
    together = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False, return_logits=True)
    assert together[0].shape == (3, 1, 60, 100)
    for i in range(3):
        alone = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes[i:i + 1], multimask_output=False, return_logits=True)
        for what, a, t in zip(("masks", "iou", "low"), alone, together):
            assert torch.equal(a, t[i:i + 1]), f"box {i}: {what} differs alone and in a batch of 3"


def test_create_sam_model_xl1_from_a_checkpoint_file_end_to_end(dev, tmp_path):
    """The reference's line, ``EfficientViTSamPredictor(create_sam_model(name="xl1", weight_url=...))``, on an xl1.pt-shaped file (seeded
    weights under "state_dict"): set_image, predict and predict_torch on the device with the reference's shapes and dtypes, with neither
    segment_anything nor torchvision imported.  bf16, since seed_encoder's weights overflow fp16 in this deep a model (see above)."""
    import sys
    from tests import sam_torch as st
    foreign = lambda: {m for m in sys.modules if m.split(".")[0] in ("segment_anything", "torchvision")}
    before = foreign()
    dt = torch.bfloat16
    src = sam.efficientvit_sam_xl1(dtype=dt, device=dev)
    seed_encoder(src.image_encoder, 4)
    pe, md = st.build()
    sd = {"prompt_encoder." + k: v for k, v in st.seed_state(pe, 1).state_dict().items()}
    sd.update({"mask_decoder." + k: v for k, v in st.seed_state(md, 2).state_dict().items()})
    missing, unexpected = src.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("image_encoder.") for k in missing)
    state = {k: v.cpu() for k, v in src.state_dict().items()}
    path = str(tmp_path / "xl1.pt")
    torch.save({"state_dict": state}, path)
    del src
    model = sam.create_sam_model(name="xl1", weight_url=path, dtype=dt, device=dev)
    assert model.image_size == (1024, 1024) and model.image_encoder.norm.eps == 1e-6 and model.mask_decoder.LN_EPS == 1e-6
    key = "image_encoder.backbone.stages.5.op_list.6.context_module.main.aggreg.0.1.weight"
    assert torch.equal(model.state_dict()[key].cpu(), state[key])
    p = sam.EfficientViTSamPredictor(model)
    image = np.random.RandomState(0).randint(0, 256, (300, 400, 3)).astype(np.uint8)
    p.set_image(image)
    assert p.features.shape == (1, 64, 64, 256) and p.input_size == (768, 1024) and p.original_size == (300, 400)
    assert torch.isfinite(p.features.float()).all()
    masks, iou, low = p.predict(box=np.array([40.0, 50.0, 300.0, 250.0]), multimask_output=False)
    assert masks.dtype == np.bool_ and masks.shape == (1, 300, 400) and iou.shape == (1,) and iou.dtype == np.float32
    assert low.shape == (1, 256, 256) and low.dtype == np.float32 and np.isfinite(low).all() and np.isfinite(iou).all()
    boxes = torch.as_tensor(p.apply_boxes(np.array([[40.0, 50.0, 300.0, 250.0], [0.0, 0.0, 399.0, 299.0]])), dtype=torch.float, device=dev)
    mt, it, lt = p.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)
    assert mt.dtype == torch.bool and mt.shape == (2, 1, 300, 400) and it.shape == (2, 1) and lt.shape == (2, 1, 256, 256) and mt.is_cuda
    assert np.array_equal(mt[0].cpu().numpy(), masks)
    assert foreign() == before                                        # nothing here imported either of them
