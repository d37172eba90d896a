"""CPU tests (-m "not gpu") of SAM's ViT image encoder, ``Sam`` and ``SamPredictor`` (omg_amd/sam_vit.py, omg_amd/segment_anything.py).

  * the oracle tests/sam_vit_torch.py against ``transformers``' SamVisionEncoder (eager attention) on the same seeded weights, on
    16 x 16 and 20 x 20 token grids whose 14 x 14 windows are padded in both axes, at head_dim 64 and 80;
  * parameter counts on the meta device against ``transformers`` and against the number derived from the layer shapes, the state-dict
    keys against the oracle's, the fixture's checksums against the regenerated weights;
  * ResizeLongestSide against hand values;
  * the new symbols are declared, bound and defined, the ABI is unchanged, the new kernels use no scratch;
  * what is refused: CPU tensors, head dims other than 64 | 80, a relative-position table of the wrong length, a mask prompt."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import omg_amd
from omg_amd import _lib, ops, sam_vit, segment_anything as sa
from tests import _codeobj
from tests import sam_vit_torch as vt
from tests import test_sam as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sam_vit_golden.npz")
NEW_SYMBOLS = ["omg_attn_relpos", "omg_gelu_erf"]
F16, BF16, F32 = _lib.OMG_F16, _lib.OMG_BF16, _lib.OMG_F32
ONE = 16                  # a non-null, 16-byte aligned stand-in address: every call below fails before any launch
BOUND = ts.BOUND          # fp32 against fp32 in another summation order, as test_sam.py's own transformers pins (max |d| / rms).  That
                          # bound counts 56 stages with sums of at most 4096 terms; the narrow encoder here has 4 blocks of 7 stages
                          # (two norms, four products, a softmax), the patch embedding and 4 neck stages (33), sums of at most 400 terms.


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


# ================================================================================================ the oracle
@pytest.mark.parametrize("dim,heads", [(128, 2), (320, 4)])
@pytest.mark.parametrize("size", [256, 320])
def test_sam_vit_torch_equals_transformers(dim, heads, size):
    from transformers.models.sam import modeling_sam as hf
    from transformers.models.sam.configuration_sam import SamVisionConfig
    cfg = SamVisionConfig(hidden_size=dim, output_channels=256, num_hidden_layers=4, num_attention_heads=heads, image_size=size, patch_size=16,
                          window_size=14, global_attn_indexes=[1, 3], mlp_dim=4 * dim, layer_norm_eps=1e-6)
    cfg._attn_implementation = "eager"
    enc = hf.SamVisionEncoder(cfg).eval()
    mine = vt.seed_vit(vt.ImageEncoderViT(size, 16, 3, dim, 4, heads, 4.0, 256, 14, (1, 3)).eval(), 3)
    mapped = {vt.hf_key(k): v for k, v in mine.state_dict().items()}
    assert set(mapped) == set(enc.state_dict()), set(mapped) ^ set(enc.state_dict())
    enc.load_state_dict(mapped, strict=True)
    x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        a, b = mine(x), enc(x).last_hidden_state
    assert a.shape == b.shape == (2, 256, size // 16, size // 16)
    e = ts.rel(a, b)
    print(f"sam_vit_torch vs transformers, D {dim}, {size // 16} x {size // 16} tokens: max |d| / rms {e:.2e} (bound {BOUND:.2e})")
    assert e <= BOUND


VARIANTS = {"vit_b": (768, 12, 12, (2, 5, 8, 11)), "vit_l": (1024, 24, 16, (5, 11, 17, 23)), "vit_h": (1280, 32, 16, (7, 15, 23, 31))}


def derived_count(D, depth, heads, glob):
    """Parameters from the layer shapes: patch embedding, pos_embed, per block two norms, qkv, proj, two tables of (2 S - 1) head_dim, the
    MLP; the neck's two convolutions without bias and two norms."""
    d = D // heads
    n = 768 * D + D + 64 * 64 * D
    for i in range(depth):
        S = 64 if i in glob else 14
        n += 2 * 2 * D + (3 * D * D + 3 * D) + (D * D + D) + 2 * (2 * S - 1) * d + (4 * D * D + 4 * D) + (4 * D * D + D)
    return n + 256 * D + 2 * 256 + 256 * 256 * 9 + 2 * 256


@pytest.mark.parametrize("name", list(VARIANTS))
def test_parameter_counts_on_the_meta_device(name):
    from transformers.models.sam import modeling_sam as hf
    from transformers.models.sam.configuration_sam import SamVisionConfig
    D, depth, heads, glob = VARIANTS[name]
    m = sam_vit.SamImageEncoderViT(embed_dim=D, depth=depth, num_heads=heads, global_attn_indexes=glob, device="meta")
    n = sum(p.numel() for p in m.parameters())
    assert n == derived_count(D, depth, heads, glob)
    with torch.device("meta"):
        enc = hf.SamVisionEncoder(SamVisionConfig(hidden_size=D, num_hidden_layers=depth, num_attention_heads=heads, global_attn_indexes=list(glob),
                                                  mlp_dim=4 * D))
    assert n == sum(p.numel() for p in enc.parameters())
    if name == "vit_h":
        assert n == 637_026_048


def test_builders_make_the_three_variants():
    assert sa.build_sam is sa.build_sam_vit_h
    assert sa.sam_model_registry == {"default": sa.build_sam_vit_h, "vit_h": sa.build_sam_vit_h, "vit_l": sa.build_sam_vit_l, "vit_b": sa.build_sam_vit_b}
    for name, (D, depth, heads, glob) in VARIANTS.items():
        m = sa.sam_model_registry[name](device="meta")
        e = m.image_encoder
        assert (e.embed_dim, len(e.blocks), e.blocks[0].attn.num_heads, e.global_attn_indexes) == (D, depth, heads, glob)
        assert [i for i, b in enumerate(e.blocks) if b.window_size == 0] == list(glob) and e.blocks[0].window_size == 14
        assert m.prompt_encoder.input_image_size == (1024, 1024) and m.mask_decoder.transformer.layers[0].mlp.lin1.weight.shape == (2048, 256)
        assert {k.split(".")[0] for k in m.state_dict()} == {"image_encoder", "prompt_encoder", "mask_decoder"}      # the pixel buffers stay out


def test_state_dict_keys_shapes_and_checkpoint_round_trip(gold, tmp_path):
    for name in ("d64", "d80"):
        ref = vt.seeded_oracle(gold, name)
        m = vt.narrow_model(gold, name)
        assert set(m.state_dict()) == set(ref.state_dict())
        assert set(m.state_dict()) == set(gold[f"{name}.sd_keys"].tolist())
        for k, v in m.state_dict().items():
            assert tuple(v.shape) == tuple(ref.state_dict()[k].shape), k
            assert np.allclose(vt.checksum(v), gold[f"{name}.sum." + k], rtol=1e-12, atol=0), k          # fp16-grid values
    # build_*(checkpoint=path): the flat fp32 state dict, strictly, every value cast to the dtype of the tensor it replaces
    ref = vt.build(128, 4, 2, (1, 3), mlp_dim=2048)
    vt.seed_vit(ref.image_encoder, 5), vt.seed_state(ref.prompt_encoder, 6), vt.seed_state(ref.mask_decoder, 7)
    path = str(tmp_path / "sam_narrow.pth")
    torch.save(ref.state_dict(), path)
    m = sa._build_sam(128, 4, 2, (1, 3), checkpoint=path)
    for k, v in m.state_dict().items():
        want = ref.state_dict()[k]
        assert v.dtype == (torch.float32 if "gaussian_matrix" in k else torch.float16), k
        assert torch.equal(v.float(), want), k                                            # seeded values lie on the fp16 grid
    bad = dict(ref.state_dict())
    bad.pop("image_encoder.pos_embed")
    torch.save(bad, path)
    with pytest.raises(RuntimeError):
        sa._build_sam(128, 4, 2, (1, 3), checkpoint=path)                                 # strict
    full = sa.build_sam_vit_b(device="meta")
    assert full.state_dict()["image_encoder.blocks.2.attn.rel_pos_h"].shape == (127, 64)
    assert full.state_dict()["image_encoder.blocks.0.attn.rel_pos_w"].shape == (27, 64)
    assert full.state_dict()["image_encoder.pos_embed"].shape == (1, 64, 64, 768)
    assert full.state_dict()["image_encoder.neck.2.weight"].shape == (256, 256, 3, 3) and "image_encoder.neck.2.bias" not in full.state_dict()


def test_exports():
    for name in ("Sam", "SamPredictor", "ResizeLongestSide", "build_sam", "build_sam_vit_h", "build_sam_vit_l", "build_sam_vit_b", "sam_model_registry"):
        assert getattr(omg_amd, name) is getattr(sa, name) and name in omg_amd.__all__
    assert omg_amd.SamImageEncoderViT is sam_vit.SamImageEncoderViT and "SamImageEncoderViT" in omg_amd.__all__
    for name in ("SamPromptEncoder", "SamMaskDecoder", "EfficientViTSam", "EfficientViTSamPredictor", "efficientvit_sam"):
        assert name in omg_amd.__all__


# ================================================================================================ the predictor's host maths
def test_resize_longest_side_against_hand_values():
    t = sa.ResizeLongestSide(1024)
    for hw, side, want in [((1024, 1024), 1024, (1024, 1024)), ((1000, 1500), 1024, (683, 1024)), ((96, 128), 1024, (768, 1024)), ((3, 1000), 512, (2, 512)),
                           ((1500, 1000), 1024, (1024, 683)), ((480, 640), 1024, (768, 1024)), ((333, 500), 1024, (682, 1024))]:
        assert sa.ResizeLongestSide.get_preprocess_shape(*hw, side) == want
    # 480 x 640 -> 768 x 1024: both axes by 1.6
    pts = np.array([[10.0, 20.0], [639.0, 479.0]])
    got = t.apply_coords(pts, (480, 640))
    assert got.dtype == np.float64 and np.allclose(got, [[16.0, 32.0], [1022.4, 766.4]], rtol=1e-15) and pts[0, 0] == 10.0
    # 1500 x 1000 -> 1024 x 683: x by 683 / 1000, y by 1024 / 1500
    got = t.apply_coords(np.array([[100.0, 300.0]]), (1500, 1000))
    assert np.array_equal(got, [[100.0 * (683 / 1000), 300.0 * (1024 / 1500)]])
    boxes = np.array([[10.0, 20.0, 110.0, 220.0], [0.0, 0.0, 640.0, 480.0]])
    assert np.allclose(t.apply_boxes(boxes, (480, 640)), [[16.0, 32.0, 176.0, 352.0], [0.0, 0.0, 1024.0, 768.0]], rtol=1e-15)
    bt = t.apply_boxes_torch(torch.tensor(boxes), (480, 640))
    assert bt.dtype == torch.float32 and bt.shape == (2, 4) and torch.allclose(bt, torch.tensor([[16.0, 32.0, 176.0, 352.0], [0.0, 0.0, 1024.0, 768.0]]))
    ct = t.apply_coords_torch(torch.tensor(pts)[None], (480, 640))
    assert ct.shape == (1, 2, 2) and torch.allclose(ct[0], torch.tensor([[16.0, 32.0], [1022.4, 766.4]]))
    img = np.random.RandomState(0).randint(0, 256, (30, 50, 3)).astype(np.uint8)
    r = sa.ResizeLongestSide(100).apply_image(img)
    assert r.shape == (60, 100, 3) and r.dtype == np.uint8 and np.array_equal(r, vt.resize_longest(img, 100))


def test_preprocess_is_segment_anythings_arithmetic(gold):
    m = vt.narrow_model(gold, "d64")
    x = torch.from_numpy(gold["image_b"]).permute(2, 0, 1)[None]
    got = m.preprocess(x)
    h, w = gold["image_b"].shape[:2]
    assert got.shape == (1, 3, 1024, 1024) and got.dtype == torch.float32
    mean, std = torch.tensor([123.675, 116.28, 103.53]).view(3, 1, 1), torch.tensor([58.395, 57.12, 57.375]).view(3, 1, 1)
    assert torch.equal(got[0, :, :h, :w], (x[0].float() - mean) / std)
    assert torch.all(got[0, :, h:, :] == 0) and torch.all(got[0, :, :, w:] == 0)
    assert "pixel_mean" not in m.state_dict()
    p = sa.SamPredictor(m)
    assert isinstance(p.transform, sa.ResizeLongestSide) and p.transform.target_length == 1024 and not p.is_image_set


# ================================================================================================ the kernels' host side
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
    assert "sam_vit.hip" in open(os.path.join(ROOT, "omg_amd", "csrc", "Makefile")).read()


def test_new_kernels_use_no_scratch():
    """Static, from the code objects in the library: every instance (f16 / bf16 x head_dim 64 / 80 x the two bias forms) without scratch
    or spills and within 256 registers, i.e. two workgroups per CU."""
    ks = _codeobj.kernels(_lib.LIB_PATH)
    inst = {n: k for n, k in ks.items() if "attn_relpos_kernel" in n}
    assert len(inst) == 8, list(inst)
    gelu = {n: k for n, k in ks.items() if "gelu_erf_kernel" in n}
    assert len(gelu) == 2, list(gelu)
    for n, k in {**inst, **gelu}.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, n
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, n
        assert k["wavefront_size"] == 64 and not k.get("uses_dynamic_stack", False), n


def relpos(dtype=F16, B=1, H=64, W=64, heads=2, d=64, window=0, qkv=ONE, ld=None, rh=ONE, rw=ONE, pad=None, out=ONE, ldo=None):
    ld = 3 * heads * d if ld is None else ld
    ldo = heads * d if ldo is None else ldo
    return _lib.lib().omg_attn_relpos(dtype, B, H, W, heads, d, window, qkv, ld, rh, rw, pad, 0.125, out, ldo, None)


@pytest.mark.parametrize("kw", [dict(d=32), dict(d=16), dict(d=72), dict(d=128), dict(dtype=F32), dict(dtype=7), dict(qkv=None), dict(rh=None), dict(rw=None),
                                dict(out=None), dict(ld=376), dict(ld=388), dict(ldo=120), dict(ldo=132), dict(qkv=ONE + 2), dict(out=ONE + 8),
                                dict(rh=ONE + 4), dict(pad=ONE + 8), dict(window=17), dict(window=-1), dict(heads=0), dict(B=-1), dict(B=70000),
                                dict(H=50, W=50), dict(H=5000, W=1), dict(H=400, W=64)])
def test_attn_relpos_rejects_bad_arguments(kw):
    """head_dim outside {64, 80}, a wrong dtype, null operands, row strides below the operand's width or off the 16-byte grid,
    misaligned pointers, a window of more than 256 positions, grid limits, bias tables beyond the LDS budget."""
    assert relpos(**kw) == -1
    assert _lib.lib().omg_last_error().decode().startswith("omg_attn_relpos:")


def test_empty_problems_and_gelu_arguments():
    lib = _lib.lib()
    assert relpos(B=0) == 0 and relpos(H=0) == 0 and relpos(W=0) == 0
    assert lib.omg_gelu_erf(F16, ONE, ONE, 12, None) == -1 and lib.omg_gelu_erf(F32, ONE, ONE, 16, None) == -1
    assert lib.omg_gelu_erf(F16, None, ONE, 16, None) == -1 and lib.omg_gelu_erf(F16, ONE, ONE + 4, 16, None) == -1
    assert lib.omg_last_error().decode().startswith("omg_gelu_erf:")
    assert lib.omg_gelu_erf(F16, ONE, ONE, 0, None) == 0


# ================================================================================================ refusals
def test_refusals(gold):
    x = torch.zeros(16, 3 * 128, dtype=torch.float16)
    t = torch.zeros(7, 64, dtype=torch.float16)
    with pytest.raises(_lib.OmgHipError):
        ops.attn_relpos(x, 1, 4, 4, 2, t, t, 0.125)                                          # CPU tensors
    with pytest.raises(_lib.OmgHipError):
        ops.gelu_erf(torch.zeros(16, dtype=torch.float16))
    with pytest.raises(_lib.OmgHipError, match="head_dim"):
        sam_vit.SamImageEncoderViT(embed_dim=96, depth=1, num_heads=2, global_attn_indexes=(), device="meta")      # head_dim 48
    with pytest.raises(_lib.OmgHipError, match="head_dim"):
        sam_vit.SamImageEncoderViT(embed_dim=256, depth=1, num_heads=2, global_attn_indexes=(), device="meta")     # head_dim 128
    m = vt.narrow_model(gold, "d64")
    with pytest.raises(_lib.OmgHipError, match="no CPU fallback"):
        m.image_encoder(torch.zeros(1, 3, 1024, 1024, dtype=torch.float16))
    # a table of another length (the reference would interpolate): refused, on any device
    a = m.image_encoder.blocks[1].attn
    a.rel_pos_h = torch.nn.Parameter(torch.zeros(63, 64, dtype=torch.float16), requires_grad=False)
    with pytest.raises(_lib.OmgHipError, match="rel_pos_h has 63 rows, the layer needs 127"):
        m.image_encoder(torch.zeros(1, 3, 1024, 1024, dtype=torch.float16))
    m = vt.narrow_model(gold, "d64")
    p = sa.SamPredictor(m)
    with pytest.raises(RuntimeError):
        p.predict(box=np.array([1.0, 2.0, 30.0, 40.0]))                                      # no image set
    with pytest.raises(RuntimeError):
        p.get_image_embedding()
    with pytest.raises(_lib.OmgHipError):
        p.set_image(gold["image_a"])                                                         # a model on the CPU
    p.is_image_set, p.original_size, p.input_size = True, (48, 64), (768, 1024)
    with pytest.raises(_lib.OmgHipError, match="mask prompt"):
        p.predict(box=np.array([1.0, 2.0, 30.0, 40.0]), mask_input=np.zeros((1, 256, 256), dtype=np.float32))
    with pytest.raises(_lib.OmgHipError, match="mask prompt"):
        p.predict_torch(boxes=torch.zeros(1, 4), mask_input=torch.zeros(1, 1, 256, 256))
