"""The DPT depth estimator without a GPU: the plain-torch oracle (tests/dpt_torch.py) against ``transformers``' class and the fixture,
the module tree of omg_amd/dpt.py against the library's on the meta device, the folded weight standardisation, the image processor,
loading from a directory, every refusal, and the static side of the new kernels."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from omg_amd import _lib
from omg_amd import dpt as hip_dpt
from tests import _codeobj
from tests import dpt_torch as dt
from tests import test_sam as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "dpt_golden.npz")
BOUND = ts.BOUND          # fp32 against fp32 in another summation order (max |d| / rms), test_sam.py's convention: its 56 stages and
                          # 4096-term sums cover this network's longest path at the fixture sizes (about 50 rounding stages, sums of
                          # at most 9 * 256 terms)
NEW_SYMBOLS = ("omg_conv3x3_nhwc_ex", "omg_dpt_stem_conv", "omg_groupnorm_res_act", "omg_maxpool3x3s2_nhwc", "omg_upsample2x_bilinear_nhwc",
               "omg_rowdot_f32", "omg_depth_tail_ws_floats", "omg_depth_tail")
NAMES = ("bit_stage1", "bit_stage2", "vit_tap0", "vit_tap1", "fused0", "fused1", "fused2", "fused3")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


def seeded(gold, name):
    cfg = dt.small_cfg(int(gold[name + ".cfg_image_size"]))
    return cfg, dt.seed_state(dt.DPTHybrid(cfg).eval(), int(gold[name + ".cfg_seed"]))


# ================================================================================================ the oracle
@pytest.mark.parametrize("name", ["s96", "s192"])
def test_dpt_torch_equals_transformers_and_the_fixture(gold, name):
    from transformers import DPTForDepthEstimation
    cfg, m = seeded(gold, name)
    sd = m.state_dict()
    assert list(gold[name + ".sd_keys"]) == list(sd)
    for k, v in sd.items():
        assert np.array_equal(dt.checksum(v), gold[f"{name}.sum.{k}"]), k
    x = torch.from_numpy(gold[name + ".input_q"].astype(np.float32) / 8.0)
    hf = DPTForDepthEstimation(dt.to_hf_config(cfg)).eval()
    hf.load_state_dict(sd, strict=True)
    m.trace = {}
    with torch.no_grad():
        mine, lib = m(x), hf(x).predicted_depth
    e = ((mine - lib).abs().max() / lib.pow(2).mean().sqrt()).item()
    print(f"dpt_torch vs transformers, {name}: max |d| / rms {e:.2e} (bound {BOUND:.2e})")
    assert e <= BOUND
    assert float((lib == 0).float().mean()) < 0.05
    i = torch.from_numpy(gold[name + ".idx.depth"])
    rec = torch.from_numpy(gold[name + ".depth"])
    assert ((lib[:, i][:, :, i] - rec).abs().max() / rec.pow(2).mean().sqrt()).item() <= BOUND
    for k in NAMES:
        i = torch.from_numpy(gold[f"{name}.idx.{k}"])
        t = m.trace[k]
        got = t[:, :, i][:, :, :, i] if t.dim() == 4 else t[:, i]
        rec = torch.from_numpy(gold[f"{name}.{k}"])
        e = ((got - rec).abs().max() / rec.pow(2).mean().sqrt()).item()
        assert e <= BOUND, (k, e)


def test_twin_rounds_and_stays_close(gold):
    cfg, m = seeded(gold, "s96")
    x = torch.from_numpy(gold["s96.input_q"].astype(np.float32) / 8.0)[:1]
    with torch.no_grad():
        ref = m(x)
        for d, cap in ((torch.float16, 2e-2), (torch.bfloat16, 1e-1)):
            e = dt.rel_rms(m(x, twin=d), ref)
            assert 0 < e < cap, (d, e)


# ================================================================================================ the module tree
def test_keys_and_parameter_count_of_dpt_hybrid_midas_on_the_meta_device():
    from transformers import DPTForDepthEstimation
    cfg = dt.full_cfg()
    with torch.device("meta"):
        hf = DPTForDepthEstimation(dt.to_hf_config(cfg))
        oracle = dt.DPTHybrid(cfg)
    mine = hip_dpt.DPTForDepthEstimation(dt.hf_config_dict(cfg), device="meta")
    want = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == want
    assert {k: tuple(v.shape) for k, v in oracle.state_dict().items()} == want
    n = sum(math.prod(s) for s in want.values())
    assert n == sum(p.numel() for p in hf.parameters()) == 122377985
    assert want["dpt.embeddings.position_embeddings"] == (1, 577, 768)
    assert all(p.dtype == torch.float16 for p in mine.parameters())


def test_exports():
    import omg_amd
    for name in ("DPTForDepthEstimation", "DPTImageProcessor", "DPTFeatureExtractor", "depth_condition"):
        assert name in omg_amd.__all__ and getattr(omg_amd, name) is getattr(hip_dpt, name)
    assert omg_amd.DPTFeatureExtractor is omg_amd.DPTImageProcessor


def test_folded_weight_standardisation_is_the_on_the_fly_form():
    from transformers.models.bit.modeling_bit import WeightStandardizedConv2d
    g = torch.Generator().manual_seed(1)
    for cin, cout, k, stride, size in ((3, 32, 7, 2, (12, 10)), (16, 16, 3, 2, (9, 8)), (16, 24, 1, 1, (5, 5)), (16, 24, 1, 2, (6, 7))):
        conv = WeightStandardizedConv2d(cin, cout, k, stride=stride, eps=1e-8, padding="same")
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.3 + 0.1)
        x = torch.randn(2, cin, *size, generator=g)
        with torch.no_grad():
            ref = conv(x)
        w = hip_dpt.fold_weight_standardization(conv.weight.data)
        assert torch.allclose(w, dt.standardize(conv.weight.data), rtol=0, atol=1e-6)
        got = F.conv2d(dt.same_pad(x, k, stride) if stride > 1 else x, w, None, stride, 0 if stride > 1 else k // 2)
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


# ================================================================================================ the image processor
@pytest.mark.parametrize("kw", [dict(size={"height": 96, "width": 96}), dict(size={"height": 64, "width": 96}, resample=2),
                                dict(size={"height": 96, "width": 96}, keep_aspect_ratio=True, ensure_multiple_of=32),
                                dict(size={"height": 80, "width": 80}, do_normalize=False), dict(do_resize=False, image_mean=[0.4, 0.5, 0.6], image_std=[0.2, 0.3, 0.25]),
                                dict(size={"height": 48, "width": 48}, do_rescale=False, do_normalize=False, resample=0)])
def test_image_processor_against_the_library(kw, tmp_path):
    from PIL import Image
    from transformers import DPTImageProcessor
    img = np.random.RandomState(2).randint(0, 256, (50, 70, 3), dtype=np.uint8)
    lib = DPTImageProcessor(**kw)
    want = lib(images=img, return_tensors="pt").pixel_values
    mine = hip_dpt.DPTImageProcessor(**kw)
    got = mine(images=img, return_tensors="pt").pixel_values
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert (got - want).abs().max().item() <= 2e-6 * max(1.0, want.abs().max().item())
    assert torch.equal(mine(images=Image.fromarray(img), return_tensors="pt")["pixel_values"], got)
    assert mine(images=[img, img], return_tensors="pt").pixel_values.shape[0] == 2
    # through a preprocessor_config.json as the library writes it
    lib.save_pretrained(tmp_path)
    again = hip_dpt.DPTFeatureExtractor.from_pretrained(tmp_path)
    assert torch.equal(again(images=img, return_tensors="pt").pixel_values, got)


# ================================================================================================ loading
@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_from_pretrained_from_a_local_directory(gold, tmp_path, fmt):
    cfg, m = seeded(gold, "s96")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    json.dump(dt.hf_config_dict(cfg), open(tmp_path / "config.json", "w"))
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(sd, str(tmp_path / "model.safetensors"))
    else:
        torch.save(sd, tmp_path / "pytorch_model.bin")
    h = hip_dpt.DPTForDepthEstimation.from_pretrained(str(tmp_path))
    assert not h.training and h.dtype == torch.float16
    for k, v in h.state_dict().items():
        assert torch.equal(v, sd[k].half()), k
    # the fold was taken from the checkpoint's own precision and survives .to()
    key = "dpt.embeddings.backbone.bit.embedder.convolution.weight"
    assert h._folded[key].dtype == torch.float32 and torch.equal(h._folded[key], dt.standardize(sd[key]))
    assert h.to(torch.bfloat16).eval().dtype == torch.bfloat16 and h._folded[key].dtype == torch.float32
    with pytest.raises(_lib.OmgHipError, match="config.json"):
        hip_dpt.DPTForDepthEstimation.from_pretrained(str(tmp_path / "nowhere"))
    os.remove(tmp_path / ("model.safetensors" if fmt == "safetensors" else "pytorch_model.bin"))
    with pytest.raises(_lib.OmgHipError, match="model.safetensors"):
        hip_dpt.DPTForDepthEstimation.from_pretrained(str(tmp_path))


# ================================================================================================ refusals
def _cfg(**kw):
    d = dt.hf_config_dict(dt.small_cfg(96))
    bb = kw.pop("backbone", None)
    d.update(kw)
    if bb:
        d["backbone_config"] = dict(d["backbone_config"], **bb)
    return d


@pytest.mark.parametrize("kw,key", [(dict(is_hybrid=False), "is_hybrid"), (dict(backbone=dict(layer_type="preactivation")), "backbone_config.layer_type"),
                                    (dict(readout_type="add"), "readout_type"), (dict(readout_type="ignore"), "readout_type"),
                                    (dict(use_batch_norm_in_fusion_residual=True), "use_batch_norm_in_fusion_residual"), (dict(add_projection=True), "add_projection"),
                                    (dict(num_attention_heads=4), "num_attention_heads"), (dict(backbone_featmap_shape=[1, 256, 8, 8]), "backbone_featmap_shape"),
                                    (dict(backbone=dict(global_padding=None)), "backbone_config.global_padding")])
def test_refusals_name_the_config_key(kw, key):
    with pytest.raises(_lib.OmgHipError, match=re.escape(f"'{key}'")):
        hip_dpt.DPTForDepthEstimation(_cfg(**kw), device="meta")


def test_refuses_the_wrong_input_size_and_the_cpu():
    h = hip_dpt.DPTForDepthEstimation(_cfg())
    with pytest.raises(_lib.OmgHipError, match="no CPU"):
        h(torch.zeros(1, 3, 96, 96))
    with pytest.raises(_lib.OmgHipError, match="do_pad"):
        hip_dpt.DPTImageProcessor(do_pad=True)


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
    assert "dpt.hip" in open(os.path.join(ROOT, "omg_amd", "csrc", "Makefile")).read()


def test_new_kernels_use_no_scratch():
    """Static, from the code objects in the library: every instance of the new kernels (and of the 3x3 convolution, whose template
    gained arguments) without scratch or spills and within 256 registers."""
    ks = _codeobj.kernels(_lib.LIB_PATH)
    want = {"stem_conv_kernel": 4, "gn_res_act_kernel": 2, "maxpool_kernel": 2, "upsample2x_kernel": 2, "rowdot_kernel": 2, "tail_minmax_kernel": 1,
            "tail_write_kernel": 1, "_114conv3x3_kernel": 12}          # the mangled length keeps dwconv3x3_kernel out
    for needle, count in want.items():
        inst = {n: k for n, k in ks.items() if needle in n}
        assert len(inst) == count, (needle, list(inst))
        for n, k in inst.items():
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, n
            assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, n
            assert k["wavefront_size"] == 64 and not k.get("uses_dynamic_stack", False), n


def test_host_side_argument_checks():
    """Refused before any launch (no GPU is touched): bad dtypes, channel counts, flags; empty problems are no-ops."""
    lib = _lib.lib()
    assert lib.omg_dpt_stem_conv(_lib.OMG_F32, _lib.OMG_F16, 16, 1, 8, 8, 24, 16, 16, None) != 0           # Cout % 32
    assert lib.omg_dpt_stem_conv(_lib.OMG_BF16, _lib.OMG_F16, 16, 1, 8, 8, 32, 16, 16, None) != 0          # pixel dtype
    assert lib.omg_conv3x3_nhwc_ex(_lib.OMG_F16, 16, 1, 4, 4, 8, 8, 1, 16, None, 3, None, 0, 16, None) != 0  # act
    assert lib.omg_conv3x3_nhwc_ex(_lib.OMG_F16, 16, 1, 4, 4, 8, 8, 1, 16, None, 0, None, 4, 16, None) != 0  # flags
    assert lib.omg_maxpool3x3s2_nhwc(_lib.OMG_F16, 16, 1, 4, 4, 12, 16, None) != 0                            # C % 8
    assert lib.omg_upsample2x_bilinear_nhwc(_lib.OMG_F32, 16, 1, 4, 4, 8, 16, None) != 0                      # dtype
    assert lib.omg_rowdot_f32(_lib.OMG_F16, 16, 32, 4, 30, 16, None, 0, 16, None) != 0                        # C % 8
    assert lib.omg_groupnorm_res_act(_lib.OMG_F16, 16, 1, 4, 24, 5, 1e-5, 16, 16, None, 0, 16, 16, None) != 0  # C % groups
    assert lib.omg_depth_tail(16, 1, 0, 4, 8, 8, 16, 16, None) != 0                                           # h == 0
    assert b"omg_depth_tail" in lib.omg_last_error()
    assert lib.omg_depth_tail(16, 0, 4, 4, 8, 8, 16, 16, None) == 0                                           # B == 0
    assert lib.omg_dpt_stem_conv(_lib.OMG_F32, _lib.OMG_F16, 16, 0, 8, 8, 32, 16, 16, None) == 0
    assert lib.omg_depth_tail_ws_floats(2, 1024, 1024) == 2 * 512 * 2
