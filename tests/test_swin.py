"""The Swin backbone without a GPU: the plain-torch oracle (tests/swin_torch.py) against the fixture and the live library class, the
loader's naming schemes, the GroundingDINO key map, the refusals, the C entry points and the new kernels' code objects."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from omg_amd import _lib
from omg_amd import swin as hip_swin
from tests import _codeobj
from tests import swin_torch as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "swin_golden.npz")
NEW_SYMBOLS = ("omg_attn_swin", "omg_swin_patch_embed", "omg_swin_merge_ln")
CONFIGS = ("w7", "w12")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


_CACHE = {}


def case(gold, name):
    """(cfg, state dict, input [2, 3, H, W], the oracle's fp32 forward) — computed once per config."""
    if name not in _CACHE:
        cfg = st.small_cfg(name)
        sd = st.seed_state(cfg, int(gold[name + ".cfg_seed"]))
        x = torch.from_numpy(gold[name + ".input_q"].astype(np.float32) / 8.0)
        with torch.no_grad():
            _CACHE[name] = (cfg, sd, x, st.forward(sd, cfg, x))
    return _CACHE[name]


def stage_names(cfg):
    return ["embeddings"] + [f"stage{i + 1}" for i in range(len(cfg["depths"]))]


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", CONFIGS)
def test_seeded_weights_are_the_fixtures(gold, name):
    cfg, sd, x, _ = case(gold, name)
    assert list(gold[name + ".sd_keys"]) == list(sd)
    assert tuple(x.shape[2:]) == cfg["image"] and np.array_equal(st.seeded_input(int(gold[name + ".cfg_input_seed"]), 2, *cfg["image"]), gold[name + ".input_q"])
    for k, v in sd.items():
        assert np.array_equal(st.checksum(v), gold[f"{name}.sum.{k}"]), k


@pytest.mark.parametrize("name", CONFIGS)
def test_oracle_equals_the_fixture(gold, name):
    """The library's numbers, recorded: every intermediate and every feature map at the stored positions, to fp32 rounding."""
    cfg, sd, x, ref = case(gold, name)
    expect = {"w7": [(23, 30), (12, 15), (6, 8)], "w12": [(26, 38), (13, 19)]}[name]
    assert ref["grids"] == expect
    for k in stage_names(cfg):
        got = ref[k][:, torch.from_numpy(gold[f"{name}.idx.{k}"])]
        assert st.rel_rms(got, torch.from_numpy(gold[f"{name}.{k}"])) < 2e-5, k
    assert len(ref["feature_maps"]) == len(cfg["out_features"])
    for n, f in enumerate(ref["feature_maps"]):
        iy, ix = (torch.from_numpy(gold[f"{name}.idx.map{n + 1}.{a}"]) for a in "yx")
        assert st.rel_rms(f[:, :, iy][:, :, :, ix], torch.from_numpy(gold[f"{name}.map{n + 1}"])) < 2e-5, n


@pytest.mark.parametrize("name", CONFIGS)
def test_oracle_equals_the_live_library(gold, name):
    transformers = pytest.importorskip("transformers")
    cfg, sd, x, ref = case(gold, name)
    hf = transformers.SwinBackbone(st.to_hf_config(cfg)).eval()
    assert list(hf.state_dict()) == list(sd)
    hf.load_state_dict(sd, strict=True)
    with torch.no_grad():
        o = hf(x, output_hidden_states=True)
    for k, h in zip(stage_names(cfg), o.hidden_states):
        assert st.rel_rms(ref[k], h.flatten(2).transpose(1, 2)) < 2e-5, k
    for a, b in zip(ref["feature_maps"], o.feature_maps):
        assert a.shape == b.shape and st.rel_rms(a, b) < 2e-5


def test_the_fixture_is_sensitive(gold):
    """Recorded by the generator, which refuses to write a fixture that cannot tell these defects from rounding."""
    for name in CONFIGS:
        for d in st.DEFECTS:
            assert float(gold[f"{name}.defect.{d}"]) >= 10.0 * float(gold[name + ".twin_err"][0]), (name, d)
    cfg, sd, x, ref = case(gold, "w12")
    with torch.no_grad():
        e = st.rel_rms(st.forward(sd, cfg, x, defect="no_shift_mask")["feature_maps"][-1], ref["feature_maps"][-1])
    assert abs(e - float(gold["w12.defect.no_shift_mask"])) <= 1e-3 * e


def test_attention_from_qkv_is_the_layers_attention():
    """The kernel tests' reference (fused QKV rows in, padded keys as pad_kv) equals the layer's literal attention (pad after the norm,
    then project): that the padded keys ARE the bias slices is what this pins."""
    torch.manual_seed(0)
    B, H, W, heads, S = 2, 9, 17, 2, 7
    C = heads * 32
    y = torch.randn(B, H * W, C, dtype=torch.float64)
    ws = [torch.randn(C, C, dtype=torch.float64) / 8 for _ in range(3)]
    bs = [torch.randn(C, dtype=torch.float64) for _ in range(3)]
    table = torch.randn((2 * S - 1) ** 2, heads, dtype=torch.float64)
    for shift in (0, 3):
        want = st.window_attention(y, H, W, S, shift, heads, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], table, lambda t: t)
        qkv = torch.nn.functional.linear(y, torch.cat(ws), torch.cat(bs)).view(B * H * W, 3 * C)
        got = st.attention_from_qkv(qkv, B, H, W, heads, S, shift, table, torch.cat(bs)[C:])
        assert float((got.view(B, H * W, C) - want).abs().max()) < 1e-12


# ------------------------------------------------------------------ loading
def module(cfg, **kw):
    return hip_swin.SwinBackbone(st.hf_config_dict(cfg), dtype=torch.float16, **kw)


def same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", CONFIGS)
def test_both_naming_schemes_and_the_groundingdino_prefix_load(gold, name):
    cfg, sd, _, _ = case(gold, name)
    a = module(cfg)
    a.load_state_dict(sd, strict=True)
    assert set(a.state_dict()) == set(sd) - {"swin.layernorm.weight", "swin.layernorm.bias"}
    assert all(torch.equal(a.state_dict()[k], sd[k].half()) for k in a.state_dict())
    hub = st.to_hub_names(sd)
    assert any(".attention.self.query." in k for k in hub) and any(".intermediate.dense." in k for k in hub) and not any("q_proj" in k for k in hub)
    hub["swin.encoder.layers.0.blocks.0.attention.self.relative_position_index"] = torch.zeros(4, dtype=torch.long)      # stored by old checkpoints: ignored
    b = module(cfg)
    b.load_state_dict(hub, strict=True)
    assert same(a.state_dict(), b.state_dict()) and same(a._pk(), b._pk())
    pre = "model.backbone.conv_encoder.model."
    det = {pre + k: v for k, v in hub.items()}
    det["model.encoder.layers.0.fusion_layer.vision_param"] = torch.zeros(3)
    c = module(cfg)
    c.load_state_dict(det, strict=True, prefix=pre)
    assert same(a.state_dict(), c.state_dict())
    with pytest.raises(_lib.OmgHipError, match="missing"):
        module(cfg).load_state_dict({k: v for k, v in sd.items() if "o_proj" not in k})
    with pytest.raises(_lib.OmgHipError, match="unexpected"):
        module(cfg).load_state_dict(dict(sd, **{"swin.encoder.layers.0.blocks.0.extra.weight": torch.zeros(1)}))
    bad = dict(sd)
    k = "swin.encoder.layers.0.blocks.0.attention.relative_position_bias.relative_position_bias_table"
    bad[k] = torch.zeros(9, sd[k].shape[1])
    with pytest.raises(_lib.OmgHipError, match="window_size"):
        module(cfg).load_state_dict(bad)


def test_library_config_objects_are_accepted():
    transformers = pytest.importorskip("transformers")
    cfg = st.small_cfg("w12")
    m = hip_swin.SwinBackbone(st.to_hf_config(cfg))
    assert m.cfg["num_heads"] == [3, 6] and m.out_features == ["stage1", "stage2"] and m.channels == [96, 192]
    gd = transformers.GroundingDinoConfig(backbone_config=transformers.SwinConfig(window_size=12, embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32],
                                                                                   out_indices=[2, 3, 4]))
    g = hip_swin.check_config(gd)
    assert g["window_size"] == 12 and g["out_features"] == ["stage2", "stage3", "stage4"] and g["depths"] == [2, 2, 18, 2]


def test_from_pretrained_reads_a_local_directory(gold, tmp_path):
    import json
    from safetensors.torch import save_file
    cfg, sd, _, _ = case(gold, "w7")
    with open(tmp_path / "config.json", "w") as f:
        json.dump(st.hf_config_dict(cfg), f)
    save_file({k: v.contiguous() for k, v in st.to_hub_names(sd).items()}, str(tmp_path / "model.safetensors"))
    m = hip_swin.SwinBackbone.from_pretrained(tmp_path)
    a = module(cfg)
    a.load_state_dict(sd)
    assert same(a.state_dict(), m.state_dict()) and not m.training
    with pytest.raises(_lib.OmgHipError, match="nothing is downloaded"):
        hip_swin.SwinBackbone.from_pretrained("microsoft/swin-base-patch4-window12-384")


@pytest.mark.parametrize("name", CONFIGS)
def test_groundingdino_key_map_round_trip(gold, name):
    """The original package is not installed, so the map is tested by round trip: the inverse renaming of a library state dict (q, k, v
    concatenated into attn.qkv, a leading ``module.``) loads to bit-identical parameters and packed weights."""
    cfg, sd, _, _ = case(gold, name)
    orig = {"module." + k: v for k, v in st.to_groundingdino_names(sd, cfg).items()}
    assert "module.backbone.0.layers.0.blocks.1.attn.qkv.weight" in orig and "module.backbone.0.norm0.weight" in orig
    assert "module.backbone.0.layers.0.downsample.reduction.weight" in orig and "module.backbone.0.patch_embed.proj.weight" in orig
    orig["module.backbone.0.layers.0.blocks.0.attn.relative_position_index"] = torch.zeros(4, dtype=torch.long)
    orig["module.transformer.level_embed"] = torch.zeros(4, 256)                                  # the rest of the detector: dropped
    orig["module.bert.embeddings.word_embeddings.weight"] = torch.zeros(4, 8)
    back = hip_swin.swin_from_groundingdino(orig)
    assert set(back) == set(sd) - {"swin.layernorm.weight", "swin.layernorm.bias"}
    assert all(torch.equal(back[k], sd[k]) for k in back)
    a, b = module(cfg), module(cfg)
    a.load_state_dict(sd)
    b.load_state_dict(back, strict=True)
    assert same(a.state_dict(), b.state_dict()) and same(a._pk(), b._pk())
    with pytest.raises(_lib.OmgHipError, match="unknown key"):
        hip_swin.swin_from_groundingdino({"backbone.0.layers.0.blocks.0.attn.gate.weight": torch.zeros(1)})


def test_packed_qkv_and_pad_kv_layout(gold):
    """Host side: the fused weight is q | k | v rows, head-major as the projections are; pad_kv is the k | v slice of the fused bias, a
    16-byte aligned view of it (what omg_attn_swin reads for a padded key)."""
    cfg, sd, _, _ = case(gold, "w12")
    m = module(cfg)
    m.load_state_dict(sd)
    pk = m._pk()
    for li, C in ((0, 96), (1, 192)):
        a = f"swin.encoder.layers.{li}.blocks.1.attention."
        w, b, pad = pk[a + "qkv.weight"], pk[a + "qkv.bias"], pk[a + "pad_kv"]
        assert tuple(w.shape) == (3 * C, C) and w.is_contiguous() and tuple(b.shape) == (3 * C,) and tuple(pad.shape) == (2 * C,)
        for i, n in enumerate("qkv"):
            assert torch.equal(w[i * C:(i + 1) * C], sd[a + f"{n}_proj.weight"].half()) and torch.equal(b[i * C:(i + 1) * C], sd[a + f"{n}_proj.bias"].half())
        assert pad.data_ptr() == b.data_ptr() + 2 * C and pad.data_ptr() % 16 == 0 and pad.is_contiguous()
        assert torch.equal(pad, torch.cat([sd[a + "k_proj.bias"], sd[a + "v_proj.bias"]]).half())
    pw = pk["patch"]
    assert tuple(pw.shape) == (96, 64) and bool((pw[:, 48:] == 0).all())
    assert torch.equal(pw[:, :48], sd["swin.embeddings.patch_embeddings.projection.weight"].half().reshape(96, 48))
    assert m._pk() is pk
    m.load_state_dict(sd)
    assert m._pk() is not pk                        # a reload rebuilds the packed operands


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("key,change", [
    ("use_absolute_embeddings", dict(use_absolute_embeddings=True)),
    ("qkv_bias", dict(qkv_bias=False)),
    ("hidden_act", dict(hidden_act="relu")),
    ("patch_size", dict(patch_size=2)),
    ("num_channels", dict(num_channels=1)),
    ("num_heads", dict(num_heads=[2, 4, 8])),                   # head_dim 16
    ("num_heads", dict(num_heads=[1, 2])),                      # fewer entries than depths
    ("window_size", dict(window_size=8)),
    ("mlp_ratio", dict(mlp_ratio=0.3)),
    ("out_features", dict(out_features=["stem"])),
    ("model_type", dict(model_type="resnet")),
])
def test_refusals_name_the_config_key(key, change):
    d = st.hf_config_dict(st.small_cfg("w7"))
    d.update(change)
    with pytest.raises(_lib.OmgHipError, match=f"'{key}'"):
        hip_swin.SwinBackbone(d)


def test_training_and_cpu_inputs_are_refused():
    m = module(st.small_cfg("w7"))
    assert not m.training
    with pytest.raises(_lib.OmgHipError, match="drop_path_rate"):
        m.train()
    with pytest.raises(_lib.OmgHipError, match="no CPU"):
        m(torch.zeros(1, 3, 32, 32))
    d = st.hf_config_dict(st.small_cfg("w7"))
    d["drop_path_rate"] = 0.2                                   # identity at inference: accepted, as the library's eval() runs it
    assert not hip_swin.SwinBackbone(d).training
    with pytest.raises(_lib.OmgHipError, match="float16 or bfloat16"):
        hip_swin.SwinBackbone(d, dtype=torch.float32)


def test_exported_from_the_package():
    import omg_amd
    assert omg_amd.SwinBackbone is hip_swin.SwinBackbone and omg_amd.swin_from_groundingdino is hip_swin.swin_from_groundingdino


# ------------------------------------------------------------------ the C side
def test_entry_points_exist():
    src = open(os.path.join(ROOT, "include", "omg_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} not declared in include/omg_hip.h"
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", nm), f"{name} is not a defined text symbol"
    assert lib.omg_abi_version() == 6
    assert "swin.hip" in open(os.path.join(ROOT, "omg_amd", "csrc", "Makefile")).read()


def test_new_kernels_use_no_scratch():
    """Static, from the code objects in the library: every instance without scratch or spills; the attention kernel within 256
    registers (two waves per SIMD, the bound the other attention kernels are held to) and within 32 KB of LDS (five workgroups per CU)."""
    ks = _codeobj.kernels(_lib.LIB_PATH)
    attn = {n: k for n, k in ks.items() if "attn_swin_kernel" in n}
    assert len(attn) == 4, list(attn)                       # f16 / bf16 x window 7 / 12
    patch = {n: k for n, k in ks.items() if "swin_patch_kernel" in n}
    merge = {n: k for n, k in ks.items() if "swin_merge_ln_kernel" in n}
    assert len(patch) == 4 and len(merge) == 8, (list(patch), list(merge))
    for n, k in {**attn, **patch, **merge}.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, n
        assert k["wavefront_size"] == 64 and not k.get("uses_dynamic_stack", False), n
    for n, k in attn.items():
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, (n, k["vgpr_count"])
        assert k["group_segment_fixed_size"] <= 32 * 1024, n


def test_host_side_argument_checks():
    """What the launcher refuses before any launch (no GPU needed: the checks come first)."""
    lib = _lib.lib()
    one = 0x1000

    def attn(dtype=0, B=1, H=8, W=8, heads=1, window=7, shift=0, qkv=one, ld=96, table=one, pad=None, out=one, ldo=32):
        return lib.omg_attn_swin(dtype, B, H, W, heads, window, shift, qkv, ld, table, pad, 0.17, out, ldo, None)

    def refused(rc, word):
        assert rc != 0 and word in lib.omg_last_error().decode(), lib.omg_last_error()

    refused(attn(dtype=2), "dtype")
    refused(attn(window=8), "window 7 or 12")
    refused(attn(shift=2), "shift")
    refused(attn(window=12, shift=3), "shift")
    refused(attn(heads=0), "heads")
    refused(attn(qkv=None), "null")
    refused(attn(ld=64), "row stride")
    refused(attn(ld=100), "multiples of 8")
    refused(attn(qkv=one + 8), "aligned")
    assert attn(B=0) == 0 and attn(H=0) == 0
    refused(lib.omg_swin_patch_embed(2, 0, one, 1, 8, 8, one, 40, None), "48")
    refused(lib.omg_swin_patch_embed(1, 0, one, 1, 8, 8, one, 64, None), "fp32 or the storage dtype")
    refused(lib.omg_swin_merge_ln(0, one, 1, 4, 4, 12, one, one, 1e-5, one, None), "multiple of 8")
    refused(lib.omg_swin_merge_ln(0, one, 1, 4, 4, 1032, one, one, 1e-5, one, None), "1024")
