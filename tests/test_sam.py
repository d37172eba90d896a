"""CPU tests (-m "not gpu") of the segmenter.

The kernels' host side (csrc/sam_decoder.hip): the entry points are declared, bound and defined, the ABI version is unchanged, every
bad argument is refused before any launch, and the wrappers refuse CPU tensors.

The module level (omg_amd/sam.py) and its oracle (tests/sam_torch.py):
  * sam_torch against ``transformers``' SamPromptEncoder / SamMaskDecoder on the same seeded weights through ``sam_torch.hf_key``;
  * the state-dict keys and shapes of omg_amd.sam's modules against the fixture of tests/golden/make_golden_sam.py, and the seeded
    decoder weights against the fixture's checksums;
  * apply_coords / apply_boxes and the preprocessing in front of the encoder against what the reference's predictor did;
  * what is refused: CPU tensors, a mask prompt, the xl names."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import omg_amd
from omg_amd import _lib, ops, sam
from tests import sam_torch as st
from tests.sam_torch import narrow_model, seeded_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["omg_attn_small", "omg_convt2x2_ln_gelu", "omg_sam_mask_logits", "omg_sam_postprocess", "omg_relu"]
F16, BF16, F32 = _lib.OMG_F16, _lib.OMG_BF16, _lib.OMG_F32
ONE = 16                  # a non-null, 16-byte aligned stand-in address: every call below fails before any launch


def test_new_symbols_in_header_bindings_and_library():
    src = open(os.path.join(ROOT, "include", "omg_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} not declared in include/omg_hip.h"
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", nm), f"{name} is not a defined text symbol"
    assert lib.omg_abi_version() == 6
    assert "sam_decoder.hip" in open(os.path.join(ROOT, "omg_amd", "csrc", "Makefile")).read()


def attn_small(dtype=F16, B=1, heads=8, d=16, Nq=7, Nk=64, q=ONE, k=ONE, v=ONE, o=ONE, ld=128, bs=0):
    return _lib.lib().omg_attn_small(dtype, B, heads, d, Nq, Nk, q, ld, bs, k, ld, bs, v, ld, bs, 0.25, o, ld, bs, None)


@pytest.mark.parametrize("kw", [dict(d=64), dict(d=8), dict(d=24), dict(Nq=0), dict(Nk=0), dict(B=0), dict(heads=0), dict(dtype=F32), dict(dtype=7),
                                dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(ld=120), dict(ld=132), dict(q=ONE + 2),
                                dict(o=ONE + 8), dict(bs=4), dict(bs=-128), dict(B=70000)])
def test_attn_small_rejects_bad_arguments(kw):
    """head_dim outside {16, 32}, empty shapes, a wrong dtype, null operands, a row stride below heads * head_dim or off the 16-byte
    grid, misaligned pointers, batch strides off the grid or negative, a batch beyond the launch grid."""
    assert attn_small(**kw) == -1
    assert _lib.lib().omg_last_error().decode().startswith("omg_attn_small:")


def convt(dtype=F16, g=ONE, ldg=256, B=1, H=4, W=4, cout=64, bias=ONE, gamma=ONE, beta=ONE, act=1, y=ONE):
    return _lib.lib().omg_convt2x2_ln_gelu(dtype, g, ldg, B, H, W, cout, bias, gamma, beta, 1e-6, act, y, None)


@pytest.mark.parametrize("kw", [dict(cout=36, ldg=144), dict(cout=4, ldg=16), dict(cout=0), dict(dtype=F32), dict(g=None), dict(y=None), dict(ldg=248),
                                dict(ldg=260), dict(gamma=None), dict(beta=None), dict(act=2), dict(H=0), dict(W=-1), dict(B=-1),
                                dict(bias=ONE + 2), dict(y=ONE + 8)])
def test_convt2x2_rejects_bad_arguments(kw):
    """Cout % 8, a wrong dtype, null operands, a row shorter than the four pieces, LayerNorm weight without bias, an unknown activation,
    empty maps, misaligned operands."""
    assert convt(**kw) == -1
    assert _lib.lib().omg_last_error().decode().startswith("omg_convt2x2_ln_gelu:")


def test_mask_logits_postprocess_and_relu_reject_bad_arguments():
    lib = _lib.lib()
    ml = lambda dtype=F16, h=ONE, u=ONE, B=1, M=4, P=65536, C=32, o=ONE: lib.omg_sam_mask_logits(dtype, h, u, B, M, P, C, o, None)
    for kw in [dict(M=5), dict(M=0), dict(C=36), dict(C=128), dict(P=0), dict(B=0), dict(dtype=F32), dict(h=None), dict(u=None), dict(o=None), dict(u=ONE + 8)]:
        assert ml(**kw) == -1, kw
    pp = lambda low=ONE, N=1, Hl=256, Wl=256, S=1024, ih=768, iw=1024, oh=96, ow=128, u8=0, o=ONE: lib.omg_sam_postprocess(low, N, Hl, Wl, S, ih, iw, oh, ow, 0.0, u8, o, None)
    for kw in [dict(low=None), dict(o=None), dict(ih=1025), dict(iw=0), dict(oh=0), dict(Hl=0), dict(S=0), dict(u8=2), dict(N=-1), dict(o=ONE + 2), dict(ow=1 << 15)]:
        assert pp(**kw) == -1, kw
    assert pp(N=0) == 0                                               # nothing to do: no launch either
    assert lib.omg_relu(F16, ONE, ONE, 12, None) == -1 and lib.omg_relu(F32, ONE, ONE, 16, None) == -1
    assert lib.omg_relu(F16, None, ONE, 16, None) == -1 and lib.omg_relu(F16, ONE, ONE + 4, 16, None) == -1
    assert lib.omg_relu(F16, ONE, ONE, 0, None) == 0


def test_wrappers_have_no_cpu_fallback():
    x = torch.zeros(1, 7, 128, dtype=torch.float16)
    with pytest.raises(_lib.OmgHipError):
        ops.attn_small(x, x, x, 8, 0.25)
    with pytest.raises(_lib.OmgHipError):
        ops.convt2x2_ln_gelu(torch.zeros(1, 2, 2, 16, dtype=torch.float16), torch.zeros(32, 16, dtype=torch.float16))
    with pytest.raises(_lib.OmgHipError):
        ops.sam_mask_logits(torch.zeros(1, 4, 32, dtype=torch.float16), torch.zeros(1, 4, 4, 32, dtype=torch.float16))
    with pytest.raises(_lib.OmgHipError):
        ops.sam_postprocess(torch.zeros(1, 1, 8, 8), 32, (32, 24), (16, 12))
    with pytest.raises(_lib.OmgHipError):
        ops.relu(torch.zeros(16, dtype=torch.float16))


def test_convt2x2_weight_packing_is_the_transposed_convolution():
    """fp32 on the CPU: rows of x against the packed weight, scattered to (2y + dy, 2x + dx), is F.conv_transpose2d(k = 2, s = 2)."""
    g = torch.Generator().manual_seed(0)
    B, cin, cout, H, W = 2, 16, 8, 3, 5
    x, w = torch.randn(B, cin, H, W, generator=g), torch.randn(cin, cout, 2, 2, generator=g)
    wp = ops.pack_convt2x2_weight(w)
    assert wp.shape == (4 * cout, cin) and wp.is_contiguous()
    rows = (x.permute(0, 2, 3, 1).reshape(-1, cin) @ wp.t()).view(B, H, W, 2, 2, cout)
    got = rows.permute(0, 5, 1, 3, 2, 4).reshape(B, cout, 2 * H, 2 * W)
    ref = torch.nn.functional.conv_transpose2d(x, w, stride=2)
    assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


# ================================================================================================ the modules and the predictor
GOLD = os.path.join(ROOT, "tests", "golden", "sam_golden.npz")

# fp32 against fp32 in another summation order.  Unit roundoff u = 2^-24.  A stage is one matrix product, softmax or normalisation whose
# rounding errors are independent of the other stages': per two-way layer 4 attentions of 4 stages each, an MLP of 2 and 4 LayerNorms
# (22), twice; the final attention and its norm (5); two upscaling layers with a norm (3); a hypernetwork of 3 and the mask product (4):
# 56.  The longest sum has 4096 terms (the softmax over the pixels), so a stage contributes at most sqrt(4096) u relative to the rms of
# its output, stages add in quadrature, and the largest of ~2 10^5 compared values lies at about 4.5 sigma.
STAGES = 56
BOUND = 4.5 * math.sqrt(STAGES) * math.sqrt(4096) * 2.0 ** -24           # 1.3e-4 of the output's rms


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


def hf_models(pe, md, size, mlp_dim):
    from transformers.models.sam import modeling_sam as hf
    from transformers.models.sam.configuration_sam import SamConfig, SamMaskDecoderConfig, SamPromptEncoderConfig, SamVisionConfig
    cfg = SamConfig(vision_config=SamVisionConfig(num_pos_feats=128, image_size=size).to_dict(),
                    prompt_encoder_config=SamPromptEncoderConfig(hidden_size=256, image_size=size, patch_size=size // 64, mask_input_channels=16).to_dict(),
                    mask_decoder_config=SamMaskDecoderConfig(hidden_size=256, mlp_dim=mlp_dim, num_hidden_layers=2, num_attention_heads=8,
                                                             iou_head_depth=3, iou_head_hidden_dim=256, layer_norm_eps=1e-5).to_dict())
    hpe, hmd = hf.SamPromptEncoder(cfg).eval(), hf.SamMaskDecoder(cfg.mask_decoder_config).eval()
    for prefix, src, dst in (("prompt_encoder", pe, hpe), ("mask_decoder", md, hmd)):
        mapped = {st.hf_key(f"{prefix}.{k}")[1]: v for k, v in src.state_dict().items()}
        assert set(mapped) == set(dst.state_dict()), (set(mapped) ^ set(dst.state_dict()))
        dst.load_state_dict(mapped, strict=True)
    return hpe, hmd


def rel(a, b):
    return (a - b).abs().max().item() / b.pow(2).mean().sqrt().item()


def test_sam_torch_equals_transformers(gold):
    size, mlp_dim = int(gold["cfg_image_size"][0]), int(gold["cfg_mlp_dim"])
    pe, md = seeded_oracle(gold)
    hpe, hmd = hf_models(pe, md, size, mlp_dim)
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(1, 256, 64, 64, generator=g)
    boxes = torch.tensor([[10.0, 8.0, 140.0, 120.5], [0.0, 0.0, 255.0, 191.0], [80.25, 90.0, 200.0, 180.0]])
    pts = torch.tensor([[[30.0, 40.0], [200.5, 20.0], [64.0, 180.0], [0.0, 0.0]], [[5.0, 6.0], [100.0, 100.0], [250.0, 190.0], [17.5, 33.0]]])
    labels = torch.tensor([[1, 0, -1, 1], [0, 1, 1, -1]], dtype=torch.int)
    worst = 0.0
    with torch.no_grad():
        dense_pe = pe.get_dense_pe()
        y, x = (torch.arange(64.0) + 0.5) / 64, (torch.arange(64.0) + 0.5) / 64
        grid = torch.stack([x[None, :].expand(64, 64), y[:, None].expand(64, 64)], dim=-1)
        hf_pe = hpe.shared_embedding(grid[None]).permute(0, 3, 1, 2)
        worst = max(worst, rel(dense_pe, hf_pe))
        cases = {"boxes": (None, boxes), "points": ((pts, labels), None), "points+boxes": ((pts, labels), boxes[:2])}
        for name, (points, bx) in cases.items():
            sparse, dense = pe(points=points, boxes=bx, masks=None)
            hs, hd = hpe(points[0][None] if points else None, points[1][None] if points else None, bx[None] if bx is not None else None, None)
            e_sparse = rel(sparse, hs[0])
            assert torch.equal(dense[0], hd[0])
            for multi in (False, True):
                low, iou = md(feat, dense_pe, sparse, dense, multi)
                hl, hi = hmd(feat, dense_pe, hs, hd, multi)
                e_low, e_iou = rel(low, hl[0]), rel(iou, hi[0])
                print(f"sam_torch vs transformers, {name}, multimask {multi}: sparse {e_sparse:.2e}  logits {e_low:.2e}  iou {e_iou:.2e}  (bound {BOUND:.2e})")
                assert low.shape == (sparse.shape[0], 3 if multi else 1, 256, 256) and iou.shape == low.shape[:2]
                worst = max(worst, e_sparse, e_low, e_iou)
    print(f"largest max |d| / rms: {worst:.3e}; bound {BOUND:.3e}")
    assert worst <= BOUND


def test_state_dict_keys_shapes_and_seeded_values(gold):
    """The modules' keys are the fixture's (the segment_anything layout), a whole checkpoint-shaped dict loads strictly, and the decoder
    weights regenerated from the fixture's seed are the ones the fixture was made with."""
    m = narrow_model(gold)
    keys = {k for k in m.state_dict() if not k.startswith("image_encoder.")}
    assert keys == set(gold["sd_keys"].tolist())
    for k in keys:
        v = m.state_dict()[k]
        assert tuple(v.shape) == tuple(gold["shape." + k]), k
        assert np.allclose(st.checksum(v), gold["sum." + k], rtol=1e-12, atol=0), k       # fp16-grid values: the sums are exact in float64 up to order
        if k.startswith("prompt_encoder."):
            assert np.array_equal(v.float().numpy(), gold["sd." + k]), k
    full = sam.efficientvit_sam("l0")
    assert {k.split(".")[0] for k in full.state_dict()} == {"image_encoder", "prompt_encoder", "mask_decoder"}
    assert full.state_dict()["mask_decoder.transformer.layers.1.mlp.lin1.weight"].shape == (2048, 256)
    assert full.state_dict()["mask_decoder.transformer.layers.0.cross_attn_token_to_image.q_proj.weight"].shape == (128, 256)
    assert full.image_size == (1024, 512) and full.prompt_encoder.input_image_size == (1024, 1024)


def test_exports():
    for name in ("SamPromptEncoder", "SamMaskDecoder", "EfficientViTSam", "EfficientViTSamPredictor", "efficientvit_sam"):
        assert getattr(omg_amd, name) is getattr(sam, name) and name in omg_amd.__all__


def test_coordinates_and_preprocessing_equal_the_reference(gold):
    m = narrow_model(gold)
    p = sam.EfficientViTSamPredictor(m)
    p._set_sizes(gold["image"].shape[:2])
    assert p.original_size == (96, 128) and p.input_size == (192, 256)
    boxes = gold["boxes"].copy()
    assert np.array_equal(p.apply_boxes(boxes), gold["boxes_in"]) and np.array_equal(boxes, gold["boxes"])
    assert np.array_equal(p.apply_coords(gold["points"]), gold["points_in"]) and p.apply_coords(gold["points"]).dtype == np.float64
    assert np.allclose(p.apply_boxes_torch(torch.from_numpy(gold["boxes"])).numpy(), gold["boxes_in"], rtol=1e-6)     # fp32 there
    resized, x = m.preprocess(gold["image"])
    assert resized is gold["image"] or np.array_equal(resized, gold["image"])                # the long side already is the encoder's
    assert x.shape == (1, 3, 128, 128) and x.dtype == torch.float32
    assert torch.equal(x[:, :, ::2, ::2], torch.from_numpy(gold["enc_in"]))
    assert torch.all(x[:, :, 96:, :] == 0)                                                   # the corner pad
    resized, x = m.preprocess(gold["image_b"])
    assert resized.dtype == np.uint8 and np.array_equal(resized, gold["resized_b"])          # bit-equal uint8 resize
    assert torch.equal(x[:, :, ::2, ::2], torch.from_numpy(gold["enc_in_b"]))
    p._set_sizes(gold["image_b"].shape[:2])
    assert p.input_size == (154, 256)
    for hw, side, want in [((1024, 1024), 1024, (1024, 1024)), ((1000, 1500), 1024, (683, 1024)), ((96, 128), 1024, (768, 1024)), ((3, 1000), 512, (2, 512))]:
        assert sam.EfficientViTSam.get_preprocess_shape(*hw, side) == want


def test_refusals(gold):
    m = narrow_model(gold)
    p = sam.EfficientViTSamPredictor(m)
    with pytest.raises(RuntimeError):
        p.predict(box=np.array([1.0, 2.0, 30.0, 40.0]))                                      # no image set
    with pytest.raises(_lib.OmgHipError):
        p.set_image(gold["image"])                                                           # a model on the CPU
    p.is_image_set = True
    p._set_sizes((96, 128))
    with pytest.raises(_lib.OmgHipError):
        p.predict(box=np.array([1.0, 2.0, 30.0, 40.0]), mask_input=np.zeros((1, 256, 256), dtype=np.float32))
    with pytest.raises(_lib.OmgHipError):
        p.predict_torch(boxes=torch.zeros(1, 4), mask_input=torch.zeros(1, 1, 256, 256))
    with pytest.raises(_lib.OmgHipError):
        m.prompt_encoder(points=None, boxes=torch.zeros(1, 4), masks=torch.zeros(1, 1, 256, 256))
    with pytest.raises(_lib.OmgHipError):
        m.prompt_encoder(points=None, boxes=torch.zeros(1, 4), masks=None)                    # a CPU tensor
    with pytest.raises(_lib.OmgHipError):
        m.mask_decoder(torch.zeros(1, 64, 64, 256, dtype=torch.float16), torch.zeros(4096, 256, dtype=torch.float16),
                       torch.zeros(1, 2, 256, dtype=torch.float16), torch.zeros(256, dtype=torch.float16), False)
    for name in ("xl0", "xl1"):
        with pytest.raises(_lib.OmgHipError):
            sam.efficientvit_sam(name)
    with pytest.raises(_lib.OmgHipError):
        sam.efficientvit_sam("l3")
