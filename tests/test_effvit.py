"""CPU tests (-m "not gpu") of the EfficientViT-SAM image encoder: the restated topology, the state-dict layout and the BatchNorm fold
against tests/golden/effvit_golden.npz (the reference's own classes in fp32, tests/golden/make_golden_effvit.py), the l0 / l1 / l2
recipes against the parameter counts of the reference's constructors, and the three new entry points of the library."""
import os

import pytest
import torch

from tests.effvit_torch import TorchEncoder, build_from_fixture, load_fixture
from omg_amd import _lib
from omg_amd.efficientvit import EfficientViTSamConfig, EfficientViTSamImageEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "effvit_golden.npz")


@pytest.fixture(scope="module")
def fixture():
    return load_fixture(GOLD)


def test_state_dict_keys_are_the_reference_layout(fixture):
    _, cfg, sd, _, _ = fixture
    m = EfficientViTSamImageEncoder(cfg, dtype=torch.float32, device="meta")
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in sd.items()}
    assert sorted(mine) == sorted(ref)
    assert mine == ref
    assert any(k.startswith("backbone.stages.0.op_list.0.conv") for k in mine) and any(k.startswith("neck.input_ops.2.op_list.0.norm") for k in mine)
    assert any(k.startswith("neck.middle.op_list.0.main.spatial_conv") for k in mine) and "neck.output_ops.0.op_list.0.conv.bias" in mine


def test_folded_weights_reproduce_every_stage_of_the_reference(fixture):
    """fp32 on the CPU: F.conv2d with the module's folded weights through the module's own tree == the reference's classes with
    BatchNorm unfolded, max |d| <= 1e-5 of each tensor's largest magnitude."""
    _, cfg, sd, vec, sub = fixture
    m = build_from_fixture(cfg, sd, torch.float32, "cpu")
    got = TorchEncoder(m, rounded=False).features(vec["x"])
    keys = [f"stage{s}" for s in range(len(cfg.width_list))] + ["neck_mid", "neck", "out"]
    assert all(k in vec for k in keys)
    for k in keys:
        g = got[k][:, :, ::sub, ::sub] if k in ("neck", "out") else got[k]
        assert g.shape == vec[k].shape, k
        rel = (g - vec[k]).abs().max().item() / vec[k].abs().max().item()
        print(f"{k}: max |d| / max |ref| = {rel:.2e}")
        assert rel <= 1e-5, (k, rel)


def test_fold_is_done_in_fp32_and_rounded_once(fixture):
    _, cfg, sd, _, _ = fixture
    m16 = build_from_fixture(cfg, sd, torch.float16, "cpu")
    m32 = build_from_fixture(cfg, sd, torch.float32, "cpu")      # the fixture's values are on the fp16 grid: same weights
    a, b = m16.backbone.stages[1].op_list[0].main.spatial_conv, m32.backbone.stages[1].op_list[0].main.spatial_conv
    w16, b16 = a.packed()
    w32, b32 = b.packed()
    assert w16.dtype == torch.float16 and w16.shape == (a.cout, 3, 3, a.cin)
    assert torch.equal(w16, w32.half()) and torch.equal(b16, b32.half())
    ref = sd["backbone.stages.1.op_list.0.main.spatial_conv.conv.weight"]
    assert not torch.equal(w32.permute(0, 3, 1, 2), ref)          # running statistics away from the identity: the fold changes the weight


@pytest.mark.parametrize("variant", ["l0", "l1", "l2"])
def test_variant_parameter_counts_match_the_reference_constructors(fixture, variant):
    g = fixture[0]
    m = EfficientViTSamImageEncoder(variant, device="meta")
    assert sum(p.numel() for p in m.parameters()) == int(g[f"params_{variant}"])
    assert m.cfg.out_dim == 256 and m.cfg.grid == 64


@pytest.mark.parametrize("variant", ["xl0", "xl1", "XL1"])
def test_xl_variants_are_refused_by_name(variant):
    with pytest.raises(_lib.OmgHipError, match="xl"):
        EfficientViTSamImageEncoder(variant, device="meta")
    with pytest.raises(_lib.OmgHipError):
        EfficientViTSamConfig.variant("b3")


def test_encoder_has_no_cpu_fallback(fixture):
    _, cfg, sd, vec, _ = fixture
    m = build_from_fixture(cfg, sd, torch.float16, "cpu")
    with pytest.raises(_lib.OmgHipError):
        m(vec["x"].half())


def test_new_entry_points_reject_bad_arguments():
    lib = _lib.lib()
    one = 16                                                          # a non-null, aligned stand-in address: every call below fails before any launch
    assert lib.omg_conv3x3_nhwc_act(_lib.OMG_F16, one, 1, 8, 8, 12, 32, 1, one, None, 0, None, one, None) == -1      # Cin = 12
    assert lib.omg_conv3x3_nhwc_act(_lib.OMG_F16, one, 1, 8, 8, 32, 36, 1, one, None, 0, None, one, None) == -1      # Cout % 8
    assert lib.omg_conv3x3_nhwc_act(_lib.OMG_F16, one, 1, 8, 8, 32, 32, 3, one, None, 0, None, one, None) == -1      # stride
    assert lib.omg_conv3x3_nhwc_act(_lib.OMG_F32, one, 1, 8, 8, 32, 32, 1, one, None, 0, None, one, None) == -1      # dtype
    assert lib.omg_dwconv3x3_act(_lib.OMG_F16, one, 12, 1, 8, 8, 12, 1, one, None, 0, one, 12, None) == -1           # C % 8
    assert lib.omg_dwconv3x3_act(_lib.OMG_F16, one, 16, 1, 8, 8, 16, 1, one, None, 4, one, 16, None) == -1           # act bits
    assert lib.omg_upsample_add_nhwc(_lib.OMG_F16, one, 1, 8, 8, 12, 64, 64, 1, one, None) == -1                     # C % 8
    assert lib.omg_upsample_add_nhwc(_lib.OMG_F16, None, 1, 8, 8, 16, 64, 64, 1, one, None) == -1                    # null
