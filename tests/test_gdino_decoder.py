"""omg_amd/gdino_decoder.py and its oracle without a GPU: tests/gdino_decoder_torch.py against tests/golden/gdino_decoder_golden.npz (made by
the installed library's own modules, tests/golden/make_golden_gdino_decoder.py), the text masks against the library's function, the
config refusals, the state-dict handling, `detect`, and the static facts of the new kernels."""
import os

import numpy as np
import pytest
import torch

from omg_amd import _lib
from omg_amd import gdino_decoder as hip
from tests import _codeobj
from tests import gdino_decoder_torch as gd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gdino_decoder_golden.npz")
CONFIGS = ["a", "b", "c"]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


def case(gold, name):
    cfg = gd.small_cfg(name)
    sd = gd.seed_state(cfg, int(gold[name + ".seed"]))
    inp = gd.seeded_inputs(cfg, int(gold[name + ".input_seed"]))
    return cfg, sd, inp


def run(cfg, sd, inp, **kw):
    with torch.no_grad():
        return gd.forward(sd, cfg, inp["memory"], inp["text"], inp["mask_flatten"], inp["text_token_mask"], inp["spatial"], inp["valid_ratios"], **kw)


@pytest.mark.parametrize("name", CONFIGS)
def test_fixture_is_the_seeded_case(gold, name):
    cfg, sd, inp = case(gold, name)
    assert list(gold[name + ".sd_keys"]) == list(sd.keys())
    from tests.golden.make_golden_gdino_decoder import NOT_APPLICABLE, checksum
    for k, v in sd.items():
        assert float(gold[f"{name}.sum.{k}"]) == float(checksum(v)), k
    assert np.array_equal(gold[name + ".memory_q"], (inp["memory"] * 8).round().to(torch.int8).numpy())
    assert np.array_equal(gold[name + ".text_q"], (inp["text"] * 8).round().to(torch.int8).numpy())
    # the generator's conditions, as recorded
    for d in gd.DEFECTS:
        if d not in NOT_APPLICABLE[name]:
            assert float(gold[f"{name}.defect.{d}"]) >= 10.0, d
    assert float(gold[name + ".gap"]) >= 20.0 * float(gold[f"{name}.twin.{'bf16' if name == 'c' else 'fp16'}.scores_maxabs"])
    if name == "a":
        assert int(gold["a.invalid_selected"]) == 1


@pytest.mark.parametrize("name", CONFIGS)
def test_oracle_reproduces_the_library(gold, name):
    cfg, sd, inp = case(gold, name)
    o = run(cfg, sd, inp)
    topk = torch.from_numpy(gold[name + ".topk"])
    assert torch.equal(o["topk_proposals"].sort(1)[0], topk.sort(1)[0]), "identical top-k sets"
    o = run(cfg, sd, inp, topk_proposals=topk)
    rows, qs = torch.from_numpy(gold[name + ".rows_s"]), torch.from_numpy(gold[name + ".q_s"])
    assert gd.rel_rms(o["scores"][:, rows], torch.from_numpy(gold[name + ".scores"])) < 1e-4
    assert gd.rel_rms(torch.stack(o["states"])[:, :, qs], torch.from_numpy(gold[name + ".states"])) < 1e-4
    assert gd.rel_rms(torch.stack(o["references"])[:, :, qs], torch.from_numpy(gold[name + ".references"])) < 1e-4
    assert gd.rel_rms(o["init_reference_points"], torch.from_numpy(gold[name + ".init_reference_points"])) < 1e-4
    assert gd.rel_rms(torch.stack(o["pred_boxes"]), torch.from_numpy(gold[name + ".pred_boxes"])) < 1e-4
    lg, want = torch.stack(o["logits"]), torch.from_numpy(gold[name + ".logits"])
    assert torch.equal(torch.isneginf(lg), torch.isneginf(want)), "exact -inf pattern"
    keep = torch.isfinite(want)
    assert gd.rel_rms(lg[keep], want[keep]) < 1e-4
    if name == "a":          # an invalid proposal is selected in sample 1: its initial reference is exactly 1
        assert bool((o["init_reference_points"][1] == 1.0).all(-1).any())


def test_every_defect_is_a_different_function(gold):
    cfg, sd, inp = case(gold, "a")
    topk = torch.from_numpy(gold["a.topk"])
    ref = run(cfg, sd, inp, topk_proposals=topk)
    for d in ("same_level_reference", "swap_sine_xy"):
        o = run(cfg, sd, inp, topk_proposals=topk, defect=d)
        assert gd.rel_rms(o["pred_boxes"][-1], ref["pred_boxes"][-1]) > 1e-3, d


def test_text_masks_are_the_librarys():
    from transformers.models.grounding_dino.modeling_grounding_dino import generate_masks_with_special_tokens_and_transfer_map as lib_masks
    rows = [
        [101, 7, 8, 9, 10, 11, 12, 13, 102, 0, 0],            # no special token inside, then padding
        [101, 7, 1012, 1012, 9, 10, 1029, 11, 12, 1012, 102],  # adjacent specials
        [101, 1012, 7, 8, 1012, 9, 102, 0, 0, 0, 0],
        [7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17],             # no special token at all
        [101, 102, 101, 102, 7, 8, 9, 1012, 10, 11, 102],
    ]
    ids = torch.tensor(rows)
    m, p = hip.text_masks_from_input_ids(ids)
    lm, lp = lib_masks(ids)
    assert torch.equal(m, lm) and torch.equal(p, lp)
    assert m.dtype == torch.bool and p.dtype == torch.long
    m1, p1 = hip.text_masks_from_input_ids(ids[1:2])
    assert torch.equal(m1, lm[1:2]) and torch.equal(p1, lp[1:2])


@pytest.mark.parametrize("key,value", [("two_stage", False), ("embedding_init_target", False), ("query_dim", 2), ("decoder_attention_heads", 4),
                                       ("decoder_n_points", 8), ("decoder_ffn_dim", 2044), ("d_model", 128), ("num_feature_levels", 5),
                                       ("activation_function", "gelu"), ("max_text_len", 512)])
def test_refusals_name_the_config_key(key, value):
    cfg = gd.small_cfg("a")
    cfg[key] = value
    with pytest.raises(_lib.OmgHipError, match=f"'{key}'"):
        hip.GroundingDinoDecoderHead(cfg)


def test_training_cpu_inputs_and_dtype_are_refused(gold):
    cfg, sd, inp = case(gold, "b")
    h = hip.GroundingDinoDecoderHead(cfg)
    with pytest.raises(_lib.OmgHipError, match="inference only"):
        h.train()
    with pytest.raises(_lib.OmgHipError, match="float16 or bfloat16"):
        hip.GroundingDinoDecoderHead(cfg, dtype=torch.float32)
    enc = type("Enc", (), dict(last_hidden_state_vision=inp["memory"], last_hidden_state_text=inp["text"], spatial_shapes_list=inp["spatial"],
                               valid_ratios=inp["valid_ratios"], mask_flatten=inp["mask_flatten"]))()
    with pytest.raises(_lib.OmgHipError, match="no CPU fallback"):
        h(enc, inp["text_token_mask"])


def test_state_dict_prefix_and_both_copies_of_the_box_heads(gold):
    cfg, sd, _ = case(gold, "a")
    h = hip.GroundingDinoDecoderHead(cfg)
    assert sorted(h.shapes()) == sorted(sd) and all(tuple(sd[k].shape) == s for k, s in h.shapes().items())
    # a GroundingDinoForObjectDetection file: everything under "model.", the box heads a second time at the top, foreign keys around
    full = {"model." + k: v for k, v in sd.items()}
    full.update({k[len("decoder."):]: v.clone() for k, v in sd.items() if k.startswith("decoder.bbox_embed.")})
    full["model.encoder.layers.0.fusion_layer.vision_param"] = torch.zeros(256)
    full["model.level_embed"] = torch.zeros(4, 256)
    assert h.load_state_dict(full, strict=True, prefix="model.") == ([], [])
    for k, v in sd.items():
        assert torch.equal(h.state_dict()[k], v.to(torch.float16)), k
    # either copy alone
    only_top = {k: v for k, v in full.items() if not k.startswith("model.decoder.bbox_embed.")}
    only_dec = {k: v for k, v in full.items() if not k.startswith("bbox_embed.")}
    for part in (only_top, only_dec):
        h2 = hip.GroundingDinoDecoderHead(cfg)
        assert h2.load_state_dict(part, strict=True, prefix="model.") == ([], [])
        assert all(torch.equal(h2.state_dict()[k], h.state_dict()[k]) for k in sd)
    # two copies that differ
    bad = dict(full)
    bad["bbox_embed.1.layers.2.bias"] = bad["bbox_embed.1.layers.2.bias"] + 1.0
    with pytest.raises(_lib.OmgHipError, match="differ"):
        hip.GroundingDinoDecoderHead(cfg).load_state_dict(bad, prefix="model.")
    # missing and unexpected keys, a wrong shape
    short = {k: v for k, v in sd.items() if k != "enc_output.bias"}
    with pytest.raises(_lib.OmgHipError, match="enc_output.bias"):
        hip.GroundingDinoDecoderHead(cfg).load_state_dict(short)
    with pytest.raises(_lib.OmgHipError, match="decoder.layers.7"):
        hip.GroundingDinoDecoderHead(cfg).load_state_dict({**sd, "decoder.layers.7.fc1.bias": torch.zeros(2048)})
    with pytest.raises(_lib.OmgHipError, match="the config needs"):
        hip.GroundingDinoDecoderHead(cfg).load_state_dict({**sd, "query_position_embeddings.weight": torch.zeros(900, 256)})


def test_from_pretrained_reads_a_local_directory(gold, tmp_path):
    import json
    from safetensors.torch import save_file
    cfg, sd, _ = case(gold, "b")
    full = {"model." + k: v.contiguous() for k, v in sd.items()}
    save_file(full, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps({k: v for k, v in cfg.items() if k not in ("grids", "padded", "name")}))
    h = hip.GroundingDinoDecoderHead.from_pretrained(tmp_path, torch_dtype=torch.bfloat16)
    assert h.dtype == torch.bfloat16 and torch.equal(h.state_dict()["enc_output.weight"], sd["enc_output.weight"].to(torch.bfloat16))
    with pytest.raises(_lib.OmgHipError, match="not a local checkpoint directory"):
        hip.GroundingDinoDecoderHead.from_pretrained(tmp_path / "nowhere")


def test_detector_from_pretrained_builds_the_four_parts_from_one_file(tmp_path):
    """A GroundingDinoForObjectDetection of the library, saved: the HIP parts load from it (the box heads from the two copies it carries)
    and the text part is the library's BERT with the file's weights."""
    import json
    from safetensors.torch import save_file
    from transformers import BertConfig, GroundingDinoConfig, SwinConfig
    from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoForObjectDetection
    bc = SwinConfig(embed_dim=32, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8], window_size=7, out_indices=[2, 3, 4])
    tc = BertConfig(hidden_size=96, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, vocab_size=1100)
    hc = GroundingDinoConfig(backbone_config=bc, text_config=tc, encoder_layers=1, decoder_layers=2, num_queries=8)
    torch.manual_seed(0)
    lib = GroundingDinoForObjectDetection(hc).eval()
    sd = {k: v.contiguous().clone() for k, v in lib.state_dict().items()}
    assert "bbox_embed.1.layers.2.weight" in sd and "model.decoder.bbox_embed.1.layers.2.weight" in sd, "the file carries the box heads twice"
    save_file(sd, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(hc.to_dict()))
    det = hip.GroundingDinoDetector.from_pretrained(tmp_path, device="cpu")
    assert isinstance(det.head, hip.GroundingDinoDecoderHead) and det.head.cfg["num_queries"] == 8 and det.head.cfg["layers"] == 2
    assert torch.equal(det.head.state_dict()["decoder.bbox_embed.1.layers.2.weight"], sd["bbox_embed.1.layers.2.weight"].half())
    assert torch.equal(det.encoder.state_dict()["level_embed"], sd["model.level_embed"].half())
    ids = torch.tensor([[101, 7, 8, 1012, 9, 102]])
    mask, pos = hip.text_masks_from_input_ids(ids)
    with torch.no_grad():
        got = det.text_backbone(ids, mask, torch.zeros_like(ids), pos)
        want = lib.model.text_backbone(ids, mask[:, None], torch.zeros_like(ids), pos)[0]
    assert torch.equal(got, want)


def test_detect_and_phrases_on_hand_made_logits():
    big, small = 4.0, -4.0                       # sigmoid: 0.982 / 0.018
    logits = torch.full((2, 3, 8), float("-inf"))
    logits[:, :, :5] = small
    logits[0, 0, 1] = big                        # sample 0, query 0: token 1
    logits[0, 2, 2], logits[0, 2, 3] = 0.0, big  # query 2: token 3 (and token 2 at 0.5: above the text threshold)
    logits[1, 1, 4] = -0.5                       # sample 1, query 1: 0.378, above a box threshold of 0.3 only
    boxes = torch.arange(24, dtype=torch.float32).view(2, 3, 4) / 24
    out = type("Out", (), dict(logits=logits, pred_boxes=boxes))()
    (b0, s0, m0), (b1, s1, m1) = hip.detect(out, box_threshold=0.3, text_threshold=0.25)
    assert torch.equal(b0, boxes[0, [0, 2]]) and torch.allclose(s0, torch.sigmoid(torch.tensor([big, big])))
    assert m0.tolist() == [[False, True] + [False] * 6, [False, False, True, True] + [False] * 4]
    assert torch.equal(b1, boxes[1, [1]]) and m1.tolist() == [[False] * 4 + [True] + [False] * 3]
    (b0, _, _), (b1, _, _) = hip.detect(out, box_threshold=0.5, text_threshold=0.25)
    assert b0.shape == (2, 4) and b1.shape == (0, 4)

    class Tok:
        def decode(self, ids):
            return " ".join(str(i) for i in ids)

    ids = torch.tensor([101, 7, 8, 9, 102])
    assert hip.phrases(m0, ids, Tok()) == ["7", "8 9"]


def test_exported_declared_and_bound():
    import omg_amd
    assert omg_amd.GroundingDinoDecoderHead is hip.GroundingDinoDecoderHead and omg_amd.GroundingDinoDetector is hip.GroundingDinoDetector
    lib = _lib.lib()
    counts = {"omg_attn_hd32": 20, "omg_msdeform_attn_box": 2, "omg_gdino_contrastive": 13, "omg_gdino_ref_step": 16}
    header = open(os.path.join(ROOT, "include", "omg_hip.h")).read()
    for n, argc in counts.items():
        assert hasattr(lib, n), n
        assert len(_lib.SYMBOLS[n][1]) == argc, n
        decl = header[header.index(f"int {n}("):]
        assert decl[:decl.index(");")].count(",") + 1 == argc, n
    assert lib.omg_abi_version() == 6
    assert "gdino_decoder.hip" in open(os.path.join(ROOT, "omg_amd", "csrc", "Makefile")).read()


def test_host_side_argument_checks():
    """Refusals that need no device: they are decided before anything is launched."""
    lib = _lib.lib()
    assert lib.omg_attn_hd32(2, 1, 8, 8, 8, None, 256, 0, None, 256, 0, None, 256, 0, None, 1.0, None, 256, 0, None) == -1
    assert b"dtype" in lib.omg_last_error()
    assert lib.omg_attn_hd32(0, 0, 8, 8, 8, None, 256, 0, None, 256, 0, None, 256, 0, None, 1.0, None, 256, 0, None) == 0       # B == 0: nothing to do
    assert lib.omg_gdino_contrastive(0, 1, 8, 300, 256, None, 256, None, 256, None, None, None, None) == -1
    assert b"max_text_len" in lib.omg_last_error()
    assert lib.omg_gdino_contrastive(0, 1, 8, 8, 256, None, 256, None, 256, None, None, None, None) == -1
    assert b"null operand" in lib.omg_last_error()
    assert lib.omg_gdino_ref_step(0, 1, 8, 5, None, None, None, None, 0, None, None, None, None, None, 0, None) == -1
    assert b"levels" in lib.omg_last_error()
    a = _lib.MsdeformArgs()
    a.dtype, a.B, a.N, a.Nq, a.heads, a.head_dim, a.L, a.points = 0, 1, 8, 8, 8, 64, 1, 4
    assert lib.omg_msdeform_attn_box(a, None) == -1 and b"head_dim 32" in lib.omg_last_error()


def test_new_kernels_use_no_scratch():
    """Static, from the code objects in the library: every instance without scratch or spills.  Recorded (vector registers incl.
    accumulation registers / LDS bytes): msdeform_box_kernel 71 .. 128 / 0; attn_hd32_kernel 88 / 9 792; gd_contrastive_kernel 84 /
    33 856 (four workgroups per CU); gd_ref_step_kernel 41 / 0."""
    ks = _codeobj.kernels(_lib.LIB_PATH)
    fam = {f: {n: k for n, k in ks.items() if f in n} for f in ("msdeform_box_kernel", "attn_hd32_kernel", "gd_contrastive_kernel", "gd_ref_step_kernel")}
    assert [len(fam[f]) for f in fam] == [16, 2, 2, 2], {f: list(v) for f, v in fam.items()}      # f16 / bf16 (x L 1..4 x mask)
    for f, inst in fam.items():
        for n, k in inst.items():
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, n
            assert k["wavefront_size"] == 64 and not k.get("uses_dynamic_stack", False), n
            assert k["vgpr_count"] + k.get("agpr_count", 0) <= 128, (n, k["vgpr_count"])
    for n, k in fam["msdeform_box_kernel"].items():
        assert k["group_segment_fixed_size"] == 0, n
    for n, k in {**fam["attn_hd32_kernel"], **fam["gd_contrastive_kernel"]}.items():
        assert k["group_segment_fixed_size"] <= 40 * 1024, n
