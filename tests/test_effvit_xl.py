"""CPU tests (-m "not gpu") of the xl EfficientViT-SAM path: the six-stage topology and its state-dict layout against
tests/golden/effvit_xl_golden.npz (the reference's own classes in fp32 after its set_norm_eps(model, 1e-6),
tests/golden/make_golden_effvit_xl.py), the xl0 / xl1 recipes against the parameter counts of the reference's constructors,
set_norm_eps and create_sam_model, LiteMLA's ``aggreg="fused"`` packing, and the new entry point of the library."""
import os
import re
import subprocess

import pytest
import torch

import omg_amd
from omg_amd import _lib, sam
from omg_amd.efficientvit import EfficientViTSamConfig, EfficientViTSamImageEncoder
from omg_amd.litemla import LiteMLA
from tests import _codeobj
from tests.effvit_xl_torch import XlTorchEncoder, build_xl, load_fixture_xl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                 # tests/test_effvit.py::test_folded_weights_reproduce_every_stage_of_the_reference: max |d| / max |ref|


@pytest.fixture(scope="module")
def fixture():
    return load_fixture_xl()


# ------------------------------------------------------------------------------------------------ topology
@pytest.mark.parametrize("variant", ["xl0", "xl1"])
def test_xl_parameter_counts_match_the_reference_constructors(fixture, variant):
    cfg = getattr(EfficientViTSamConfig, variant)()
    assert cfg.fused_aggreg and cfg.block_list[4:] == ("att@3", "att@3") and len(cfg.width_list) == 6 and cfg.neck_fids == (5, 4, 3)
    m = EfficientViTSamImageEncoder(cfg, device="meta")
    assert sum(p.numel() for p in m.parameters()) == int(fixture[0][f"params_{variant}"])
    mlas = [x for x in m.modules() if isinstance(x, LiteMLA)]
    assert len(mlas) == cfg.depth_list[4] + cfg.depth_list[5] and all(x.scales == (3,) and x.fused_aggreg and x.dim == 32 for x in mlas)
    assert len(m.backbone.stages[0].op_list) == 1 + cfg.depth_list[0]


def test_by_name_refusal_points_to_the_xl_builders():
    for call in (lambda: EfficientViTSamConfig.variant("xl1"), lambda: EfficientViTSamImageEncoder("xl0", device="meta"), lambda: sam.efficientvit_sam("xl1")):
        with pytest.raises(_lib.OmgHipError, match="xl") as e:
            call()
        assert "efficientvit_sam_xl0" in str(e.value) and "create_sam_model" in str(e.value)


def test_narrow_state_dict_is_the_reference_layout_and_loads_strictly(fixture):
    _, cfg, sd, _, _ = fixture
    assert cfg.depth_list[0] == 0 and cfg.block_list[4] == "att@3"
    m = EfficientViTSamImageEncoder(cfg, dtype=torch.float32, device="cpu")
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in sd.items()}
    assert sorted(mine) == sorted(ref) and mine == ref
    assert "backbone.stages.5.op_list.1.context_module.main.aggreg.0.0.weight" in mine
    assert mine["backbone.stages.5.op_list.1.context_module.main.aggreg.0.0.weight"][-2:] == (3, 3)
    assert "backbone.stages.4.op_list.0.main.depth_conv.conv.bias" in mine          # the att stages downsample with an MBConv (fewer_norm)
    assert not any(k.startswith("backbone.stages.0.op_list.1") for k in mine)       # depth_list[0] == 0: the stem alone
    m.load_state_dict(sd, strict=True)


def rel_errors(m, vec, sub, cfg):
    got = XlTorchEncoder(m, rounded=False).features(vec["x"])
    keys = [f"stage{s}" for s in range(len(cfg.width_list))] + ["neck_mid", "neck", "out"]
    assert all(k in vec for k in keys)
    out = {}
    for k in keys:
        g = got[k][:, :, ::sub, ::sub] if k in ("neck", "out") else got[k]
        assert g.shape == vec[k].shape, k
        out[k] = (g - vec[k]).abs().max().item() / vec[k].abs().max().item()
    return out


def test_folded_weights_at_eps_1e6_reproduce_every_stage_of_the_reference(fixture):
    """fp32 on the CPU, after set_norm_eps(model, 1e-6): every fixture tensor to fp32 rounding (the l-series test's tolerance).  The
    same model without the call misses by a wide margin, and a model that was packed before the call still hits: the cache is dropped."""
    _, cfg, sd, vec, sub = fixture
    m = build_xl(cfg, sd, torch.float32, "cpu", eps=1e-6)
    assert m.norm.eps == 1e-6 and m.backbone.stages[0].op_list[0].norm.eps == 1e-6
    for k, rel in rel_errors(m, vec, sub, cfg).items():
        print(f"eps 1e-6 {k}: max |d| / max |ref| = {rel:.2e}")
        assert rel <= TOL, (k, rel)

    plain = build_xl(cfg, sd, torch.float32, "cpu", eps=None)
    miss = rel_errors(plain, vec, sub, cfg)
    print("eps 1e-5 (no set_norm_eps):", {k: f"{v:.2e}" for k, v in miss.items()})
    assert all(v > 100 * TOL for v in miss.values()), miss

    late = build_xl(cfg, sd, torch.float32, "cpu", eps=None)
    layers = [l for l in late.modules() if hasattr(l, "packed")]
    mlas = [l for l in late.modules() if isinstance(l, LiteMLA)]
    for l in layers:
        late._pk(l)                                                   # packed at eps = 1e-5 ...
    stale = [l._pk()["wproj"].clone() for l in mlas]
    assert late._packed and all(l._packed for l in mlas)
    sam.set_norm_eps(late, 1e-6)                                      # ... and dropped here
    assert not late._packed and not any(l._packed for l in mlas)
    conv = late.backbone.stages[1].op_list[0].main.spatial_conv
    assert torch.equal(late._pk(conv)[0], m._pk(m.backbone.stages[1].op_list[0].main.spatial_conv)[0])
    assert any(not torch.equal(l._pack()["wproj"], s) for l, s in zip(mlas, stale))
    for k, rel in rel_errors(late, vec, sub, cfg).items():
        assert rel <= TOL, (k, rel)


# ------------------------------------------------------------------------------------------------ create_sam_model, set_norm_eps
def narrow_sam(cfg, dtype=torch.float32):
    return sam.EfficientViTSam(EfficientViTSamImageEncoder(cfg, dtype=dtype, device="cpu"), sam.SamPromptEncoder(256, (64, 64), (128, 128), 16, dtype=dtype),
                               sam.SamMaskDecoder(256, 3, 2, 8, 128, 3, 256, dtype=dtype), image_size=(128, 128))


def check_eps(model, eps):
    enc, md = model.image_encoder, model.mask_decoder
    bns = [m for m in enc.modules() if type(m).__name__ == "_BatchNorm"]
    mlas = [m for m in enc.modules() if isinstance(m, LiteMLA)]
    assert bns and mlas
    assert all(m.eps == eps for m in bns) and enc.norm.eps == eps and all(m.proj.norm.eps == eps for m in mlas) and md.LN_EPS == eps


def test_set_norm_eps_reaches_every_norm_but_the_upscaling_layernorm2d(fixture, monkeypatch):
    _, cfg, _, _, _ = fixture
    model = narrow_sam(cfg)
    check_eps(model, 1e-5)
    md = model.mask_decoder
    md._packed = {"stale": True}
    sam.set_norm_eps(model, 1e-6)
    check_eps(model, 1e-6)
    assert md._packed is None and sam.SamMaskDecoder.LN_EPS == 1e-5 and "LN_EPS" in vars(md)      # an instance attribute; the class default stays
    # the decoder's LayerNorms run at LN_EPS, the upscaling LayerNorm2d at its own 1e-6, whatever set_norm_eps was given
    seen = []
    monkeypatch.setattr(sam.ops, "layernorm", lambda x, w, b, eps: seen.append(eps) or x)
    md._norm(torch.zeros(1, 2, 256), md.transformer.norm_final_attn)
    assert seen == [1e-6]
    sam.set_norm_eps(model, 1e-3)
    md._norm(torch.zeros(1, 2, 256), md.transformer.norm_final_attn)
    assert seen == [1e-6, 1e-3]
    import inspect
    src = inspect.getsource(sam.SamMaskDecoder.forward_features)
    assert "ln_weight=ln.weight.data, ln_bias=ln.bias.data, eps=1e-6" in src                       # output_upscaling.1: a literal, not LN_EPS


def test_create_sam_model_names_and_errors():
    with pytest.raises(ValueError, match="b3"):
        sam.create_sam_model("b3", pretrained=False)
    with pytest.raises(ValueError, match="xl2"):
        sam.create_sam_model("xl2-foo", weight_url="nowhere.pt")
    with pytest.raises(ValueError, match="weight"):
        sam.create_sam_model("xl1")                                   # pretrained=True and no weight_url: no model zoo directory here
    with pytest.raises(ValueError, match="weight"):
        sam.create_sam_model("l0", pretrained=True, weight_url=None)
    assert omg_amd.create_sam_model is sam.create_sam_model


@pytest.mark.parametrize("name,variant", [("xl0", "xl0"), ("xl1-foo", "xl1"), ("l0", None)])
def test_create_sam_model_builds_by_name_with_eps_1e6(name, variant):
    model = sam.create_sam_model(name, pretrained=False, device="meta")
    assert isinstance(model, sam.EfficientViTSam)
    if variant is not None:
        assert model.image_encoder.cfg == getattr(EfficientViTSamConfig, variant)() and model.image_size == (1024, 1024)
        assert model.prompt_encoder.input_image_size == (1024, 1024) and model.prompt_encoder.image_embedding_size == (64, 64)
    else:
        assert model.image_encoder.cfg == EfficientViTSamConfig.variant("l0") and model.image_size == (1024, 512)
    check_eps(model, 1e-6)
    assert model.mask_decoder.iou_token.weight.dtype == torch.float16


@pytest.mark.parametrize("wrapped", [False, True])
def test_create_sam_model_loads_a_checkpoint_file(fixture, tmp_path, monkeypatch, wrapped):
    """A round trip through torch.save of a narrow model's state dict, bare and under "state_dict"; eps is 1e-6 afterwards."""
    _, cfg, sd, _, _ = fixture
    src = narrow_sam(cfg, torch.float16)
    src.image_encoder.load_state_dict({k: (v.half() if v.dtype.is_floating_point and "running" not in k else v) for k, v in sd.items()})
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in list(src.prompt_encoder.parameters()) + list(src.mask_decoder.parameters()):
            p.copy_(torch.randn(p.shape, generator=g).half())
    state = {k: v.clone() for k, v in src.state_dict().items()}
    path = str(tmp_path / "xl0.pt")
    torch.save({"state_dict": state, "epoch": 3} if wrapped else state, path)
    monkeypatch.setattr(sam, "efficientvit_sam_xl0", lambda dtype=torch.float16, device=None: narrow_sam(cfg, dtype))
    model = sam.create_sam_model("xl0-narrow", weight_url=path)
    got = model.state_dict()
    assert sorted(got) == sorted(state) and all(torch.equal(got[k], state[k]) for k in state)
    check_eps(model, 1e-6)
    assert not model.image_encoder._packed


def test_public_names_are_exported():
    for name in ("efficientvit_sam_xl0", "efficientvit_sam_xl1", "create_sam_model", "set_norm_eps"):
        assert getattr(omg_amd, name) is getattr(sam, name) and name in omg_amd.__all__
    assert omg_amd.EfficientViTSamConfig is EfficientViTSamConfig and omg_amd.EfficientViTSamImageEncoder is EfficientViTSamImageEncoder
    m = sam.efficientvit_sam_xl1(image_size=1024, device="meta")
    assert m.image_size == (1024, 1024) and m.image_encoder.cfg.head_depth == 12
    assert sam.efficientvit_sam_xl0(device="meta").image_encoder.cfg.head_depth == 6


def test_predictor_sizes_with_equal_image_size_entries(fixture):
    """preprocess, _set_sizes and postprocess_masks's frame for image_size = (S, S) (the reference's sam.py:225-300): the long side is
    resized to S, input_size is the resized image's size, and the padded input is S x S."""
    _, cfg, _, _, _ = fixture
    model = narrow_sam(cfg)
    p = sam.EfficientViTSamPredictor(model)
    p._set_sizes((60, 100))
    assert p.original_size == (60, 100) and p.input_size == (77, 128)
    import numpy as np
    resized, x = model.preprocess(np.zeros((60, 100, 3), dtype=np.uint8))
    assert resized.shape == (77, 128, 3) and x.shape == (1, 3, 128, 128) and resized.shape[:2] == p.input_size
    assert torch.all(x[:, :, 77:] == 0) and torch.all(x[:, :, :77] != 0)
    p._set_sizes((128, 96))
    assert p.input_size == (128, 96) and model.preprocess(np.zeros((128, 96, 3), dtype=np.uint8))[0].shape == (128, 96, 3)


# ------------------------------------------------------------------------------------------------ LiteMLA(aggreg="fused")
@pytest.mark.parametrize("dim", [16, 32])
def test_litemla_fused_packs_no_block_diagonal_image(dim):
    from oracle import litemla as ol
    sd = ol.init_state_dict(64, 64, dim, scales=(3,), seed=2, dtype=torch.float16)
    fused = LiteMLA(64, 64, dim=dim, scales=(3,), aggreg="fused", device="cpu")
    gemm = LiteMLA(64, 64, dim=dim, scales=(3,), device="cpu")
    assert sorted(fused.state_dict()) == sorted(gemm.state_dict()) == sorted(list(sd) + ["proj.norm.num_batches_tracked"])     # the reference's keys
    sd["proj.norm.num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    fused.load_state_dict(sd, strict=True)
    gemm.load_state_dict(sd, strict=True)
    pf, pg = fused._pack(), gemm._pack()
    assert fused.fused_aggreg and "wbd" not in pf and len(pf["wg"]) == 1 and "wg" not in pg and len(pg["wbd"]) == 1
    T3 = 3 * 64
    assert pf["wg"][0].shape == (T3, dim) and pg["wbd"][0].shape == (T3, T3)
    assert torch.equal(pf["wg"][0], sd["aggreg.0.1.weight"].reshape(T3, dim))
    assert pf["wg"][0].data_ptr() == fused.aggreg[0][1].weight.data_ptr()                 # the checkpoint's own tensor: no derived image
    for g in range(T3 // dim):                                                            # and the image the GEMM path builds holds the same blocks
        assert torch.equal(pg["wbd"][0][g * dim:(g + 1) * dim, g * dim:(g + 1) * dim], pf["wg"][0][g * dim:(g + 1) * dim])
    assert torch.equal(pf["taps"][0], pg["taps"][0]) and torch.equal(pf["wproj"], pg["wproj"])


def test_litemla_fused_with_dim_8_falls_back_to_the_gemm_path():
    m = LiteMLA(32, 32, dim=8, scales=(5,), aggreg="fused", device="cpu")
    torch.nn.init.normal_(m.qkv.conv.weight)
    for a in m.aggreg:
        torch.nn.init.normal_(a[0].weight), torch.nn.init.normal_(a[1].weight)
    torch.nn.init.normal_(m.proj.conv.weight)
    pk = m._pack()
    assert not m.fused_aggreg and "wg" not in pk and pk["wbd"][0].shape == (96, 96)
    with pytest.raises(_lib.OmgHipError):
        LiteMLA(32, 32, dim=8, aggreg="fuse")


# ------------------------------------------------------------------------------------------------ the library
def test_new_symbol_in_header_bindings_and_library():
    name = "omg_litemla_aggreg"
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "omg_hip.h")).read(), flags=re.S)
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(rf"\b{name}\s*\(", src), f"{name} not declared in include/omg_hip.h"
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(rf"\bT {name}\b", nm), f"{name} is not a defined text symbol"
    assert lib.omg_abi_version() == 6
    from omg_amd import ops
    assert callable(ops.litemla_aggreg)


def test_new_entry_point_rejects_bad_arguments():
    lib = _lib.lib()
    one, far = 1 << 20, 1 << 30                                      # non-null, aligned stand-in addresses: every call below fails before any launch
    F16 = _lib.OMG_F16
    call = lambda dtype=F16, X=one, ldx=96, B=1, H=4, W=4, C=96, k=3, dim=32, Wt=far, Wg=far, Y=far + (1 << 20), ldy=96: \
        lib.omg_litemla_aggreg(dtype, X, ldx, B, H, W, C, k, dim, Wt, Wg, Y, ldy, None)
    assert call(dim=8) == -1 and call(dim=24) == -1                  # dim 8 stays on the GEMM path
    assert call(C=80) == -1                                          # C % dim
    assert call(k=4) == -1 and call(k=11) == -1
    assert call(dtype=_lib.OMG_F32) == -1
    assert call(ldx=88) == -1 and call(ldy=100) == -1
    assert call(X=None) == -1 and call(Wg=None) == -1 and call(X=one + 8) == -1
    assert call(Y=one) == -1                                         # in place
    assert call(ldx=192, ldy=192, Y=one + 2 * 48) == -1              # overlapping columns of the same buffer
    assert call(ldx=192, Y=one + 2 * 96, ldy=96) == -1               # the same memory under another row stride
    assert call(B=0) == 0                                            # nothing to do


def test_aggreg_kernels_use_no_scratch_and_do_not_spill():
    ks = _codeobj.kernels(_lib.LIB_PATH)
    inst = {n: k for n, k in ks.items() if "aggreg_kernel" in n}
    assert len(inst) == 4, list(inst)                                # f16 / bf16 x dim 16 / 32
    for n, k in inst.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, n
        assert k["wavefront_size"] == 64 and not k.get("uses_dynamic_stack", False), n
