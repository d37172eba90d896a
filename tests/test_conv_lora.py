"""LoRA on convolution layers, CPU side (-m "not gpu"): the float64 merge helper pinned against torch, the file loaders in all three key
styles, the ABI of omg_conv2d_slots and the code objects of its kernel instantiations."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from omg_amd import loaders
from omg_amd.lora import LoraAdapter
from omg_amd.unet import UNet2DConditionModel, UNetConfig
from tests import _codeobj
from tests import _conv_lora_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("OMG_CODEOBJ_LIB") or os.path.join(ROOT, "omg_amd", "csrc", "libomg_hip.so")


# ------------------------------------------------------------------ the merge helper
@pytest.mark.parametrize("k,stride", [(1, 1), (3, 1), (3, 2)])
def test_merge_helper_is_what_torch_computes(k, stride):
    """``F.conv2d(F.conv2d(x, A, stride, padding), B)`` — PEFT's Conv2d LoRA layer: lora_B(lora_A(x)) with lora_A = Conv2d(Cin, r, k, stride,
    padding) and lora_B = Conv2d(r, Cout, 1) — equals the helper's unmerged form and a conv with its merged delta weight, to 1e-12."""
    g = torch.Generator().manual_seed(k * 10 + stride)
    cin, cout, r, pad = 6, 10, 4, k // 2
    x = torch.randn(2, cin, 9, 7, generator=g, dtype=torch.float64)
    A = torch.randn(r, cin, k, k, generator=g, dtype=torch.float64)
    B = torch.randn(cout, r, generator=g, dtype=torch.float64)
    want = F.conv2d(F.conv2d(x, A, stride=stride, padding=pad), B[:, :, None, None])
    assert (co.unmerged(x, A, B, stride=stride, padding=pad) - want).abs().max() < 1e-12
    assert (co.unmerged(x, A, B[:, :, None, None], stride=stride, padding=pad) - want).abs().max() < 1e-12
    assert (F.conv2d(x, co.delta_weight(A, B), stride=stride, padding=pad) - want).abs().max() < 1e-12
    W = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
    full = F.conv2d(x, W, stride=stride, padding=pad) + 0.8 * want
    assert (F.conv2d(x, co.merged_weight(W, [(A, B, 0.8)]), stride=stride, padding=pad) - full).abs().max() < 1e-12
    xn = x.permute(0, 2, 3, 1)
    if k == 3 or stride == 1:
        assert (co.conv_nhwc(xn, W, stride=stride, extra=0.8 * co.lora_nhwc(xn, A, B, stride=stride)).permute(0, 3, 1, 2) - full).abs().max() < 1e-12


@pytest.mark.parametrize("k,stride", [(1, 1), (3, 1), (3, 2)])
def test_merge_helper_against_the_peft_layer(k, stride):
    peft = pytest.importorskip("peft")
    from peft.tuners.lora.layer import Conv2d as PeftConv2d
    torch.manual_seed(0)
    base = torch.nn.Conv2d(6, 10, k, stride=stride, padding=k // 2).double()
    layer = PeftConv2d(base, "default", r=4, lora_alpha=8, lora_dropout=0.0, init_lora_weights=False).double()
    x = torch.randn(2, 6, 9, 7, dtype=torch.float64)
    A, B = layer.lora_A["default"].weight.data, layer.lora_B["default"].weight.data
    want = layer(x)
    got = base(x) + 2.0 * co.unmerged(x, A, B, stride=stride, padding=k // 2)
    assert (got - want).abs().max() < 1e-12


# ------------------------------------------------------------------ loaders
@pytest.fixture(scope="module")
def tiny():
    return UNet2DConditionModel(UNetConfig.tiny(), device="meta")


CONV_MODS = ["down_blocks.0.resnets.0.conv1", "down_blocks.1.resnets.0.conv2", "down_blocks.1.resnets.0.conv_shortcut",
             "down_blocks.0.downsamplers.0.conv", "up_blocks.0.upsamplers.0.conv", "mid_block.resnets.1.conv1"]
LIN_MODS = ["down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q", "mid_block.attentions.0.transformer_blocks.0.ff.net.2"]


def make_adapter(unet, ranks=(4, 4), alpha=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    convs = loaders.conv_module_paths(unet)
    w = {}
    for i, mod in enumerate(LIN_MODS):
        lin = unet.get_submodule(mod)
        r = ranks[i % 2]
        w[mod] = (torch.randn(r, lin.in_features, generator=g), torch.randn(lin.out_features, r, generator=g))
    for i, mod in enumerate(CONV_MODS):
        cin, cout, k = convs[mod]
        r = ranks[i % 2]
        w[mod] = (torch.randn(r, cin, k, k, generator=g), torch.randn(cout, r, generator=g))
    return LoraAdapter("c", w, alpha=alpha)


def test_conv_module_paths_lists_the_slot_convs_only(tiny):
    convs = loaders.conv_module_paths(tiny)
    assert "conv_in" not in convs and "conv_out" not in convs
    assert all(m in convs for m in CONV_MODS)
    assert convs["down_blocks.1.resnets.0.conv_shortcut"] == (64, 128, 1) and convs["down_blocks.0.downsamplers.0.conv"] == (64, 64, 3)


@pytest.mark.parametrize("style", ["peft", "diffusers", "kohya"])
def test_round_trip_with_conv_entries(tiny, style):
    ad = make_adapter(tiny, ranks=(4, 8))                     # mixed ranks
    sd = loaders.lora_state_dict(ad, style)
    up_keys = [k for k in sd if "conv" in k and (k.endswith("lora_B.weight") or k.endswith("up.weight"))]
    assert up_keys and all(sd[k].dim() == 4 and tuple(sd[k].shape[2:]) == (1, 1) for k in up_keys)      # files hold the up weight as a 1x1 conv
    got = loaders.load_lora_adapter(tiny, sd, "c")
    assert set(got.weights) == set(ad.weights) and got.rank == 8
    for mod, (a, b) in ad.weights.items():
        ga, gb = got.weights[mod]
        assert torch.equal(ga, a) and torch.equal(gb, b), mod
        assert got.scaling(mod) == 1.0


def test_kohya_sgm_names_of_convolutions(tiny):
    """SGM block naming of a resnet conv, a shortcut, a downsampler and an upsampler (kohya-ss's SDXL trainer with conv_dim)."""
    convs = loaders.conv_module_paths(tiny)
    names = {"input_blocks_1_0_in_layers_2": "down_blocks.0.resnets.0.conv1", "input_blocks_4_0_out_layers_3": "down_blocks.1.resnets.0.conv2",
             "input_blocks_4_0_skip_connection": "down_blocks.1.resnets.0.conv_shortcut", "input_blocks_3_0_op": "down_blocks.0.downsamplers.0.conv",
             "output_blocks_2_2_conv": "up_blocks.0.upsamplers.0.conv", "middle_block_2_in_layers_2": "mid_block.resnets.1.conv1"}
    g = torch.Generator().manual_seed(1)
    sd, want = {}, {}
    for flat, mod in names.items():
        cin, cout, k = convs[mod]
        a, b = torch.randn(4, cin, k, k, generator=g), torch.randn(cout, 4, 1, 1, generator=g)
        sd[f"lora_unet_{flat}.lora_down.weight"], sd[f"lora_unet_{flat}.lora_up.weight"] = a, b
        sd[f"lora_unet_{flat}.alpha"] = torch.tensor(2.0)
        want[mod] = (a, b.reshape(cout, 4) * (2.0 / 4))                 # alpha / r folded into the up matrix
    got = loaders.load_lora_adapter(tiny, sd, "k")
    assert set(got.weights) == set(want)
    for mod, (a, b) in want.items():
        assert torch.equal(got.weights[mod][0], a) and torch.allclose(got.weights[mod][1], b, rtol=0, atol=0), mod


def test_alpha_is_folded_per_layer_with_mixed_ranks(tiny):
    ad = make_adapter(tiny, ranks=(4, 8), alpha=2.0)
    got = loaders.load_lora_adapter(tiny, loaders.lora_state_dict(ad, "kohya"), "c")
    for mod, (a, b) in ad.weights.items():
        assert torch.equal(got.weights[mod][1], b.reshape(b.shape[0], -1) * (2.0 / a.shape[0])), mod


def _sd(tiny, mod="down_blocks.0.resnets.0.conv1", r=4):
    cin, cout, k = loaders.conv_module_paths(tiny)[mod]
    return {f"unet.{mod}.lora_A.weight": torch.zeros(r, cin, k, k), f"unet.{mod}.lora_B.weight": torch.zeros(cout, r, 1, 1)}, mod


def test_loader_refuses_by_name(tiny):
    sd, mod = _sd(tiny)
    loaders.load_lora_adapter(tiny, sd, "ok")
    # a down kernel that is not the base layer's
    bad = dict(sd); bad[f"unet.{mod}.lora_A.weight"] = torch.zeros(4, 64, 1, 1)
    with pytest.raises(loaders.LoaderError, match="down kernel"):
        loaders.load_lora_adapter(tiny, bad, "x")
    # an up that is not 1x1
    bad = dict(sd); bad[f"unet.{mod}.lora_B.weight"] = torch.zeros(64, 4, 3, 3)
    with pytest.raises(loaders.LoaderError, match="1x1"):
        loaders.load_lora_adapter(tiny, bad, "x")
    # conv_in / conv_out, in every key style
    for key_a, key_b in (("unet.conv_in.lora_A.weight", "unet.conv_in.lora_B.weight"), ("unet.conv_out.lora.down.weight", "unet.conv_out.lora.up.weight"),
                         ("lora_unet_conv_in.lora_down.weight", "lora_unet_conv_in.lora_up.weight"),
                         ("lora_unet_input_blocks_0_0.lora_down.weight", "lora_unet_input_blocks_0_0.lora_up.weight"),
                         ("lora_unet_out_2.lora_down.weight", "lora_unet_out_2.lora_up.weight")):
        bad = dict(sd); bad[key_a] = torch.zeros(4, 4, 3, 3); bad[key_b] = torch.zeros(64, 4, 1, 1)
        with pytest.raises(loaders.LoaderError, match="conv_in / conv_out"):
            loaders.load_lora_adapter(tiny, bad, "x")
    # other adapter algebras are named, not skipped
    for key in ("lora_unet_input_blocks_1_0_in_layers_2.hada_w1_a", "lora_unet_input_blocks_1_0_in_layers_2.lokr_w1",
                "lora_unet_input_blocks_1_0_in_layers_2.lora_mid.weight", "lora_unet_input_blocks_1_0_in_layers_2.dora_scale",
                f"unet.{mod}.lora_magnitude_vector"):
        bad = dict(sd); bad[key] = torch.zeros(4, 4)
        with pytest.raises(loaders.LoaderError, match="LoHa / LoKr / Tucker"):
            loaders.load_lora_adapter(tiny, bad, "x")
    # half a pair
    bad = dict(sd); del bad[f"unet.{mod}.lora_B.weight"]
    with pytest.raises(loaders.LoaderError):
        loaders.load_lora_adapter(tiny, bad, "x")


def test_parse_without_conv_paths_still_refuses_conv_targets(tiny):
    sd, _ = _sd(tiny)
    with pytest.raises(loaders.LoaderError, match="not a Linear"):
        loaders.parse_lora_state_dict(sd, loaders.linear_module_paths(tiny))
    with pytest.raises(loaders.LoaderError, match="conv layers is not supported"):
        loaders.parse_lora_state_dict({"lora_unet_input_blocks_1_0_in_layers_2.lora_down.weight": torch.zeros(4, 64, 3, 3),
                                       "lora_unet_input_blocks_1_0_in_layers_2.lora_up.weight": torch.zeros(64, 4, 1, 1)}, loaders.linear_module_paths(tiny))


def test_synthetic_adapter_draws_conv_targets_after_the_linear_ones():
    from omg_amd.lora import lora_conv_target_names, lora_target_names, make_synthetic_adapter
    unet = UNet2DConditionModel(UNetConfig.tiny(), device="cpu")
    plain = make_synthetic_adapter(unet, "a", 4, seed=7)
    both = make_synthetic_adapter(unet, "a", 4, seed=7, conv=True)
    assert set(plain.weights) == set(lora_target_names(unet))
    assert set(both.weights) == set(lora_target_names(unet)) | set(lora_conv_target_names(unet))
    for k, (a, b) in plain.weights.items():                       # the Linear draws (the benchmark's weights) do not depend on `conv`
        assert torch.equal(both.weights[k][0], a) and torch.equal(both.weights[k][1], b)
    k = "down_blocks.0.downsamplers.0.conv"
    assert tuple(both.weights[k][0].shape) == (4, 64, 3, 3) and tuple(both.weights[k][1].shape) == (64, 4)


# ------------------------------------------------------------------ ABI
def test_slots_struct_size_matches_the_header_and_the_abi_version_stays():
    from omg_amd import _lib
    code = '#include <stdio.h>\n#include "omg_hip.h"\nint main(){printf("%zu %zu %d\\n",sizeof(omg_conv2d_slots_args),sizeof(omg_conv2d_args),OMG_ABI_VERSION);return 0;}'
    exe = os.path.join(ROOT, "tests", "_sizes_conv_slots.out")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=code.encode(), check=True)
    try:
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    finally:
        os.remove(exe)
    assert out == [ctypes.sizeof(_lib.Conv2dSlotsArgs), ctypes.sizeof(_lib.Conv2dArgs), 6]
    assert _lib.Conv2dSlotsArgs.conv.offset == 0
    assert _lib.lib().omg_abi_version() == 6
    assert "omg_conv2d_slots" in _lib.SYMBOLS and hasattr(_lib.lib(), "omg_conv2d_slots")


# ------------------------------------------------------------------ code objects
@pytest.mark.skipif(not _codeobj.available(LIB), reason="libomg_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_the_segment_form_of_the_conv_kernel_uses_no_scratch():
    """gemm_kernel<T, CONV = true, GLDS, CSEG = true> — the only instantiations omg_conv2d_slots adds (fp16 / bf16 x LDS-DMA / register staged):
    no scratch, no spills, and still two blocks per CU (at most 256 registers per lane).  The slot launches without a segment reuse the
    CONV instantiations omg_conv2d launches; none of those may use scratch either."""
    ks = _codeobj.kernels(LIB)
    seg = {n: k for n, k in ks.items() if re.search(r"11gemm_kernelIDF16b?_?Lb1ELb[01]ELb1EEEv", n)}
    assert len(seg) == 4, sorted(seg)
    for n, k in seg.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256 and k["max_flat_workgroup_size"] == 256, (n, k)
    # every CONV instantiation a slot launch can reach, counted per kernel family (fp16 + bf16): the 128x128 kernel {LDS-DMA, register staged} x
    # {plain, CSEG}, v6 256x{256,128}, v7 256x256 and 128x320, the four epilogue forms of v12, the three of v13
    conv = {n: k for n, k in ks.items() if re.search(r"gemm_kernel(_v\d+)?IDF16b?_?Lb1E", n)}
    fam = {}
    for n in conv:
        f = re.search(r"gemm_kernel(_v\d+)?I", n).group(1) or "v1"
        fam[f] = fam.get(f, 0) + 1
    assert fam == {"v1": 8, "_v6": 4, "_v7": 4, "_v12": 8, "_v13": 6}, fam
    for n, k in conv.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
