"""omg_amd.BertTextEncoder without a GPU (-m "not gpu"): the plain-torch oracle tests/bert_torch.py against tests/golden/bert.npz (the
library's BertModel in fp32 under GroundingDINO's block mask and per-phrase positions), the module's state-dict handling, its fused
q | k | v pack, its refusals, the two entries of the C ABI and the detector's ``text_backbone`` keyword."""
import json
import os
import re

import numpy as np
import pytest
import torch

from omg_amd import _lib as L
from omg_amd import bert as hip_bert
from omg_amd import gdino_decoder as hip
from tests import bert_torch as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bert.npz")
CASES = [(n, T) for n in ("a", "b") for T in bt.small_cfg(n)["lengths"]]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


def checksum(v: torch.Tensor) -> float:
    return float((v.double() * torch.arange(1, v.numel() + 1, dtype=torch.float64).reshape(v.shape).remainder(7.0).add(1.0)).sum())


def inputs_of(gold, name, T):
    P = f"{name}.T{T}."
    return dict(input_ids=torch.from_numpy(gold[P + "input_ids"]), token_type_ids=torch.from_numpy(gold[P + "token_type_ids"]),
                attention_mask=torch.from_numpy(gold[P + "attention_mask"]).bool(), position_ids=torch.from_numpy(gold[P + "position_ids"]))


_SD = {}


def state(gold, name):
    if name not in _SD:
        _SD[name] = bt.seed_state(bt.small_cfg(name), int(gold[name + ".cfg_seed"]))
    return _SD[name]


@pytest.mark.parametrize("name", ["a", "b"])
def test_seed_state_regenerates_the_fixtures_weights(gold, name):
    sd = state(gold, name)
    assert list(sd) == [str(k) for k in gold[name + ".sd_keys"]]
    for k, v in sd.items():
        assert checksum(v) == pytest.approx(float(gold[f"{name}.sum.{k}"]), rel=1e-12, abs=1e-9), k


@pytest.mark.parametrize("name,T", CASES)
def test_oracle_matches_the_fixture(gold, name, T):
    """The fixture's conditions (tests/golden/make_golden_bert.py) hold in the file, the inputs regenerate, the masks are those of the
    module's own text_masks_from_input_ids, and the oracle reproduces the library's recorded states to fp32 rounding."""
    cfg, sd, inp = bt.small_cfg(name), state(gold, name), inputs_of(gold, name, T)
    P = f"{name}.T{T}."
    again = bt.seeded_ids(cfg, T, 1000 * int(gold[name + ".cfg_seed"]) + T)
    for k in inp:
        assert torch.equal(again[k], inp[k]), k
    mask, pos = hip.text_masks_from_input_ids(inp["input_ids"])
    assert torch.equal(mask, inp["attention_mask"]) and torch.equal(pos, inp["position_ids"])
    lens = [int(x) for x in gold[P + "lengths"]]
    assert len(set(lens)) == 3 and max(lens) == T
    assert any(int(t) in (1012, 1029) for t in inp["input_ids"][0]) and int(inp["token_type_ids"].max()) == 1
    with torch.no_grad():
        states = bt.forward(sd, cfg, **inp)
    it, ic = torch.from_numpy(gold[P + "idx.token"]), torch.from_numpy(gold[P + "idx.channel"])
    assert len(states) == cfg["layers"] + 1
    for i, s in enumerate(states):
        e = bt.rel_rms(s[:, it][:, :, ic], torch.from_numpy(gold[P + f"state{i}"]))
        assert e < 2e-5, (i, e)
    assert float(gold[P + "oracle_err"].max()) < 2e-5
    t16 = float(gold[P + "twin_err"][0, -1])
    for d in bt.DEFECTS:
        assert float(gold[P + f"defect.{d}"]) >= 10.0 * t16, d


def hf_sd(cfg, seed=5, extra=True):
    sd = {k: v for k, v in bt.seed_state(cfg, seed).items()}
    if extra:
        sd["pooler.dense.weight"], sd["pooler.dense.bias"] = torch.zeros(cfg["hidden"], cfg["hidden"]), torch.zeros(cfg["hidden"])
        sd["embeddings.position_ids"] = torch.arange(cfg["positions"])[None]
    return sd


TINY = dict(hidden=128, heads=2, inter=72, layers=2, vocab=40, positions=16, types=2, eps=1e-12)


def test_state_dict_keys_load_with_and_without_the_prefix():
    sd = hf_sd(TINY)
    m = hip_bert.BertTextEncoder(bt.hf_config_dict(TINY), dtype=torch.float16)
    assert m.load_state_dict(sd) == ([], [])
    own = m.state_dict()
    assert sorted(own) == sorted(bt.shapes(TINY)) and not [k for k in own if k.startswith("pooler.") or k.endswith("position_ids")]
    for k in own:
        assert torch.equal(own[k], sd[k].half()), k
    pre = "model.text_backbone."
    big = {pre + k: v for k, v in sd.items()}
    big["model.level_embed"] = torch.zeros(4, 256)                  # another module's key: ignored
    m2 = hip_bert.BertTextEncoder(bt.hf_config_dict(TINY), dtype=torch.bfloat16)
    assert m2.load_state_dict(big, prefix=pre) == ([], [])
    assert torch.equal(m2.state_dict()["encoder.layer.1.output.dense.weight"], sd["encoder.layer.1.output.dense.weight"].bfloat16())


def test_unknown_missing_and_misshapen_keys_are_reported():
    m = hip_bert.BertTextEncoder(bt.hf_config_dict(TINY))
    sd = hf_sd(TINY)
    sd["encoder.layer.0.attention.self.distance_embedding.weight"] = torch.zeros(3, 3)
    with pytest.raises(L.OmgHipError, match="unexpected.*distance_embedding"):
        m.load_state_dict(sd)
    sd = hf_sd(TINY)
    del sd["encoder.layer.1.intermediate.dense.bias"]
    with pytest.raises(L.OmgHipError, match="missing.*encoder.layer.1.intermediate.dense.bias"):
        m.load_state_dict(sd)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert missing == ["encoder.layer.1.intermediate.dense.bias"] and unexpected == []
    sd = hf_sd(TINY)
    sd["embeddings.LayerNorm.weight"] = torch.zeros(64)
    with pytest.raises(L.OmgHipError, match=r"embeddings.LayerNorm.weight is \(64,\)"):
        m.load_state_dict(sd)


def test_the_fused_qkv_pack_is_the_three_weights_stacked():
    sd = hf_sd(TINY)
    m = hip_bert.BertTextEncoder(bt.hf_config_dict(TINY))
    m.load_state_dict(sd)
    pk = m._pk()
    for i in range(TINY["layers"]):
        p = f"encoder.layer.{i}.attention.self."
        for s in ("weight", "bias"):
            want = torch.cat([sd[p + n + "." + s] for n in ("query", "key", "value")], 0).half()
            assert torch.equal(pk[p + "qkv." + s], want) and pk[p + "qkv." + s].is_contiguous(), (i, s)
        assert pk[p + "qkv.weight"].shape == (3 * TINY["hidden"], TINY["hidden"])
    m.load_state_dict({k: v + 1 for k, v in sd.items()})
    assert not torch.equal(m._pk()["encoder.layer.0.attention.self.qkv.bias"], pk["encoder.layer.0.attention.self.qkv.bias"]), "a stale pack"


@pytest.mark.parametrize("change,key", [
    (dict(num_attention_heads=4), "num_attention_heads"),          # head_dim 32
    (dict(hidden_act="relu"), "hidden_act"),
    (dict(hidden_act="gelu_new"), "hidden_act"),
    (dict(position_embedding_type="relative_key"), "position_embedding_type"),
    (dict(is_decoder=True), "is_decoder"),
    (dict(add_cross_attention=True), "add_cross_attention"),
    (dict(hidden_size=132, num_attention_heads=2), "hidden_size"),
    (dict(intermediate_size=68), "intermediate_size"),
])
def test_refusals_name_the_config_key(change, key):
    cfg = dict(bt.hf_config_dict(TINY), **change)
    with pytest.raises(L.OmgHipError, match=f"config key '{key}'"):
        hip_bert.BertTextEncoder(cfg)


def test_training_dtype_and_linear_are_refused():
    m = hip_bert.BertTextEncoder(bt.hf_config_dict(TINY))
    assert not m.training
    with pytest.raises(L.OmgHipError, match="training"):
        m.train()
    with pytest.raises(L.OmgHipError, match="dtype"):
        hip_bert.BertTextEncoder(bt.hf_config_dict(TINY), dtype=torch.float32)
    with pytest.raises(L.OmgHipError, match="linear"):
        hip_bert.BertTextEncoder(bt.hf_config_dict(TINY), linear="cublas")
    assert m.uses_skinny(hip_bert.T_SKINNY) and not m.uses_skinny(hip_bert.T_SKINNY + 1)
    assert hip_bert.BertTextEncoder(bt.hf_config_dict(TINY), linear="skinny").uses_skinny(256)
    assert not hip_bert.BertTextEncoder(bt.hf_config_dict(TINY), linear="gemm").uses_skinny(4)


def test_too_many_tokens_are_refused_with_the_key():
    m = hip_bert.BertTextEncoder(bt.hf_config_dict(TINY))                         # 16 positions
    ids = torch.zeros(1, 17, dtype=torch.long)
    with pytest.raises(L.OmgHipError, match="config key 'max_position_embeddings'.*17 tokens.*16 rows"):
        m(ids)
    m = hip_bert.BertTextEncoder(dict(bt.hf_config_dict(TINY), max_position_embeddings=512))
    ids = torch.zeros(1, 257, dtype=torch.long)
    with pytest.raises(L.OmgHipError, match="config key 'max_position_embeddings'.*257 tokens.*at most 256"):
        m(ids)
    with pytest.raises(L.OmgHipError, match="no CPU fallback"):
        m(torch.zeros(1, 4, dtype=torch.long))


def test_the_library_exports_both_entries_and_the_header_declares_them():
    l = L.lib()                  # raises when the library is not built or a declared symbol is missing
    assert l.omg_abi_version() == 6
    for name in ("omg_gemm_skinny", "omg_bert_embed_ln"):
        assert name in L.SYMBOLS and getattr(l, name) is not None
    header = open(os.path.join(ROOT, "include", "omg_hip.h")).read()
    assert re.search(r"#define\s+OMG_ABI_VERSION\s+6\b", header)
    for name, nargs in (("omg_gemm_skinny", 15), ("omg_bert_embed_ln", 18)):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert m is not None, name
        assert len(m.group(1).split(",")) == nargs == len(L.SYMBOLS[name][1]), name
    assert "clamped" in header.lower()


def _detector_checkpoint(tmp_path):
    from safetensors.torch import save_file
    from transformers import BertConfig, GroundingDinoConfig, SwinConfig
    from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoForObjectDetection
    bc = SwinConfig(embed_dim=32, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8], window_size=7, out_indices=[2, 3, 4])
    tc = BertConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, vocab_size=1100)
    hc = GroundingDinoConfig(backbone_config=bc, text_config=tc, encoder_layers=1, decoder_layers=2, num_queries=8)
    torch.manual_seed(0)
    lib = GroundingDinoForObjectDetection(hc).eval()
    sd = {k: v.contiguous().clone() for k, v in lib.state_dict().items()}
    save_file(sd, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(hc.to_dict()))
    return sd


def test_detector_from_pretrained_builds_the_hip_text_encoder(tmp_path):
    sd = _detector_checkpoint(tmp_path)
    det = hip.GroundingDinoDetector.from_pretrained(tmp_path, device="cpu", text_backbone="hip")
    import omg_amd
    assert isinstance(det.text_backbone, omg_amd.BertTextEncoder) and det.text_backbone is not None
    t = det.text_backbone
    assert t.dtype == torch.float16 and t.cfg["hidden"] == 128 and t.cfg["heads"] == 2 and t.cfg["layers"] == 1 and t.linear == "auto"
    pre = "model.text_backbone."
    own = t.state_dict()
    mine = [k for k in sd if k.startswith(pre) and not k[len(pre):].startswith("pooler.") and not k.endswith("position_ids")]
    assert sorted(own) == sorted(k[len(pre):] for k in mine) and len(own) == 5 + 16
    for k in mine:
        assert torch.equal(own[k[len(pre):]], sd[k].half()), k
    assert isinstance(det.head, hip.GroundingDinoDecoderHead)
    bf = hip.GroundingDinoDetector.from_pretrained(tmp_path, torch_dtype=torch.bfloat16, device="cpu", text_backbone="hip")
    assert bf.text_backbone.dtype == torch.bfloat16
    alone = hip_bert.BertTextEncoder.from_pretrained(tmp_path, device="cpu", linear="skinny")
    assert alone.linear == "skinny" and alone.t_skinny == hip_bert.T_SKINNY
    assert hip_bert.BertTextEncoder.from_pretrained(tmp_path, device="cpu", t_skinny=64).t_skinny == 64
    assert torch.equal(alone.state_dict()["embeddings.LayerNorm.bias"], own["embeddings.LayerNorm.bias"])


def test_an_unknown_text_backbone_and_a_missing_directory_raise(tmp_path):
    with pytest.raises(L.OmgHipError, match="text_backbone='onnx'"):
        hip.GroundingDinoDetector.from_pretrained(tmp_path, device="cpu", text_backbone="onnx")
    with pytest.raises(L.OmgHipError, match="BertTextEncoder.from_pretrained.*not a local checkpoint directory"):
        hip_bert.BertTextEncoder.from_pretrained(tmp_path / "nowhere")


def test_a_plain_bert_checkpoint_loads_from_the_top_level_of_its_config(tmp_path):
    from safetensors.torch import save_file
    sd = hf_sd(TINY, extra=True)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(dict(bt.hf_config_dict(TINY), model_type="bert")))
    m = hip_bert.BertTextEncoder.from_pretrained(tmp_path, device="cpu", prefix="")
    assert m.cfg["inter"] == 72 and torch.equal(m.state_dict()["embeddings.word_embeddings.weight"], sd["embeddings.word_embeddings.weight"].half())
