"""Makes tests/golden/gdino_decoder_golden.npz (CPU only; a few minutes, most of it the seed search).

The reference is the installed transformers library's own GroundingDinoForObjectDetection modules in fp32 — generate_encoder_output_proposals,
encoder_output_class_embed, encoder_output_bbox_embed, query_position_embeddings, the GroundingDinoDecoder, class_embed / bbox_embed —
composed exactly as GroundingDinoModel.forward ("Fifth, prepare decoder inputs" on) and the head loop of
GroundingDinoForObjectDetection.forward compose them, starting from seeded encoder outputs.

The weights are NOT stored: tests/gdino_decoder_torch.py's ``seed_state`` regenerates them from the recorded seed and the per-key
checksums pin them.  The encoder outputs are stored as int8 (value = q / 8).

Per config (gdino_decoder_torch.small_cfg):
  seed, input_seed                      the seeds
  sd_keys, sum.<key>                    the state-dict keys and a float64 checksum per key
  memory_q, text_q                      the encoder outputs as int8
  topk                                  the library's top-k proposals [B, Q]; rows_s / scores: the selection scores at sampled rows
  q_s                                   the sampled queries; states [layers, B, len(q_s), 256], references [layers, B, len(q_s), 4],
                                        init_reference_points [B, Q, 4]
  logits [levels, B, Q, max_text_len], pred_boxes [levels, B, Q, 4]
  twin.<dtype>.<what>                   rel_rms of the oracle's 16-bit twin against the library (last state, all states, references,
                                        pred_boxes, finite logits) and the maximum absolute error of its selection scores
  defect.<name>                         the largest of (rel_rms of the defective oracle against the library) / (the fp16 twin's figure)
                                        over pred_boxes, the last state and the finite logits

Conditions, asserted here (the search runs over input seeds until they hold); they are conditions on the fixture, not tolerances:
  1. every defect that applies to the config moves pred_boxes, the last state or the logits by at least 10 x the fp16 twin's figure;
  2. in every sample the library's gap between the selection scores ranked num_queries and num_queries + 1 is at least 20 x the fp16
     twin's maximum absolute error on the scores (configs a and b), so the selected SET is decided by the model and not by rounding;
     for bf16 the same holds on a config of its own, c (b with 6 queries): at rank 19 of 319 a gap of 20 bf16 errors is nine mean
     spacings of the scores in both samples at once, and no input seed in 20 000 has it; a's and b's bf16 cases take the library's
     top-k as an input;
  3. in config a at least one selected proposal of sample 1 is an invalid one (box logit +inf): all 59 padded rows of that sample share
     one score and are selected together, so condition 2's gap lies between valid rows.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import gdino_decoder_torch as gd  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gdino_decoder_golden.npz")
CONFIGS = {"a": dict(seed=61, first_input_seed=1000, dtype=torch.float16), "b": dict(seed=62, first_input_seed=2000, dtype=torch.float16),
           "c": dict(seed=63, first_input_seed=3000, dtype=torch.bfloat16)}
SENSITIVITY, GAP = 10.0, 20.0
# config b has no padding.  no_logit_eps changes a result only where a reference is exactly 0 or 1 (config a's invalid proposals), and
# there by sigmoid(delta + 11.5) against 1: 1e-5 on a coordinate, below what 16-bit storage resolves; omg_gdino_ref_step's own test
# (float64, references of exactly 0 and 1) is what sees it
NOT_APPLICABLE = {"a": ("no_logit_eps",), "b": ("no_text_key_mask", "no_value_mask", "valid_ratio_one", "no_logit_eps")}
NOT_APPLICABLE["c"] = NOT_APPLICABLE["b"]
MAX_SEEDS = 20000


def pick(n, k):
    return np.unique(np.round(np.linspace(0, n - 1, min(n, k))).astype(np.int64))


def checksum(v: torch.Tensor) -> np.ndarray:
    return np.array(float((v.double() * torch.arange(1, v.numel() + 1, dtype=torch.float64).reshape(v.shape).remainder(7.0).add(1.0)).sum()))


def library_model(cfg, sd):
    from transformers import BertConfig, GroundingDinoConfig, SwinConfig
    from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoForObjectDetection
    bc = SwinConfig(embed_dim=32, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8], window_size=7, out_indices=[2, 3, 4])
    tc = BertConfig(hidden_size=96, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, vocab_size=64)
    hc = GroundingDinoConfig(backbone_config=bc, text_config=tc, encoder_layers=1, decoder_layers=cfg["decoder_layers"],
                             num_queries=cfg["num_queries"], d_model=cfg["d_model"], decoder_attention_heads=cfg["decoder_attention_heads"],
                             decoder_ffn_dim=cfg["decoder_ffn_dim"], decoder_n_points=cfg["decoder_n_points"],
                             num_feature_levels=cfg["num_feature_levels"], layer_norm_eps=cfg["layer_norm_eps"], max_text_len=cfg["max_text_len"],
                             decoder_bbox_embed_share=cfg["decoder_bbox_embed_share"], two_stage=True, embedding_init_target=True)
    det = GroundingDinoForObjectDetection(hc).eval()
    own = det.model.state_dict()
    assert all(k in own and tuple(own[k].shape) == tuple(v.shape) for k, v in sd.items()), [k for k in sd if k not in own]
    det.model.load_state_dict(sd, strict=False)
    full = det.state_dict()
    for k, v in sd.items():                     # the detection model carries the box heads twice: both copies hold the seeded tensors
        assert torch.equal(full["model." + k], v), k
        if k.startswith("decoder.bbox_embed."):
            assert torch.equal(full[k[len("decoder."):]], v), k
    return det


def library_select(det, inp):
    m = det.model
    oq, prop = m.generate_encoder_output_proposals(inp["memory"], ~inp["mask_flatten"], inp["spatial"])
    cls = m.encoder_output_class_embed(oq, inp["text"], inp["text_token_mask"])
    return oq, prop, cls.max(-1)[0]


def library_run(det, cfg, inp):
    """-> dict like the oracle's."""
    m, Q = det.model, cfg["num_queries"]
    B = inp["memory"].shape[0]
    with torch.no_grad():
        oq, prop, scores = library_select(det, inp)
        coord = m.encoder_output_bbox_embed(oq) + prop
        topk = torch.topk(scores, Q, dim=1)[1]
        ref = torch.gather(coord, 1, topk.unsqueeze(-1).repeat(1, 1, 4)).sigmoid()
        target = m.query_position_embeddings.weight.unsqueeze(0).repeat(B, 1, 1)
        sp = torch.as_tensor(inp["spatial"], dtype=torch.long)
        lsi = torch.cat((sp.new_zeros((1,)), sp.prod(1).cumsum(0)[:-1]))
        dec = m.decoder(inputs_embeds=target, vision_encoder_hidden_states=inp["memory"], vision_encoder_attention_mask=inp["mask_flatten"],
                        text_encoder_hidden_states=inp["text"], text_encoder_attention_mask=~inp["text_token_mask"], reference_points=ref,
                        spatial_shapes=sp, spatial_shapes_list=inp["spatial"], level_start_index=lsi, valid_ratios=inp["valid_ratios"],
                        self_attn_mask=None, return_dict=True)
        hs, irs = dec.intermediate_hidden_states, dec.intermediate_reference_points
        logits, boxes = [], []
        for level in range(hs.shape[1]):
            reference = torch.special.logit(ref if level == 0 else irs[:, level - 1], eps=1e-5)
            logits.append(det.class_embed[level](vision_hidden_state=hs[:, level], text_hidden_state=inp["text"], text_token_mask=inp["text_token_mask"]))
            boxes.append((det.bbox_embed[level](hs[:, level]) + reference).sigmoid())
    return dict(scores=scores, topk_proposals=topk, init_reference_points=ref, states=tuple(hs.unbind(1)), references=tuple(irs.unbind(1)),
                logits=tuple(logits), pred_boxes=tuple(boxes), prop=prop)


def oracle(cfg, sd, inp, **kw):
    with torch.no_grad():
        return gd.forward(sd, cfg, inp["memory"], inp["text"], inp["mask_flatten"], inp["text_token_mask"], inp["spatial"], inp["valid_ratios"], **kw)


def rounded(sd, dtype):
    return {k: v.to(dtype).float() for k, v in sd.items()}


def finite_pair(a, b):
    keep = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), keep)
    return a[keep], b[keep]


def selection_ok(det, cfg, rsd, inp, dtype, name):
    """Conditions 2 and 3 on one input seed, from the selection alone."""
    Q = cfg["num_queries"]
    with torch.no_grad():
        _, prop, scores = library_select(det, inp)
        tw = oracle(cfg, rsd, inp, twin=dtype, scores_only=True)["scores"]
    err = float((tw - scores).abs().max())
    top = torch.sort(scores, dim=1, descending=True)[0]
    gap = float((top[:, Q - 1] - top[:, Q]).min())
    ok = gap >= GAP * err
    if ok and name == "a":
        topk = torch.topk(scores, Q, dim=1)[1]
        ok = bool(torch.isinf(torch.gather(prop, 1, topk.unsqueeze(-1).repeat(1, 1, 4))[1]).any())
    return ok, gap, err


def search(det, cfg, sd, first, dtype, name):
    rsd = rounded(sd, dtype)
    for s in range(first, first + MAX_SEEDS):
        inp = gd.seeded_inputs(cfg, s)
        ok, gap, err = selection_ok(det, cfg, rsd, inp, dtype, name)
        if ok:
            print(f"  config {name} {dtype}: input seed {s}, gap {gap:.4f}, twin score error {err:.5f}")
            return s, inp, gap, err
    return -1, None, 0.0, 0.0


def figures(o, lib):
    lg_o, lg_l = finite_pair(torch.stack(o["logits"]), torch.stack(lib["logits"]))
    return dict(last_state=gd.rel_rms(o["states"][-1], lib["states"][-1]), states=gd.rel_rms(torch.stack(o["states"]), torch.stack(lib["states"])),
                references=gd.rel_rms(torch.stack(o["references"]), torch.stack(lib["references"])),
                pred_boxes=gd.rel_rms(torch.stack(o["pred_boxes"]), torch.stack(lib["pred_boxes"])), logits=gd.rel_rms(lg_o, lg_l))


def build():
    out = {}
    for name, c in CONFIGS.items():
        P = name + "."
        cfg = gd.small_cfg(name)
        sd = gd.seed_state(cfg, c["seed"])
        det = library_model(cfg, sd)
        seed, inp, gap, err = search(det, cfg, sd, c["first_input_seed"], c["dtype"], name)
        assert seed >= 0, f"config {name}: no input seed in {MAX_SEEDS} meets conditions 2 and 3"
        lib = library_run(det, cfg, inp)
        topk = lib["topk_proposals"]
        ref = oracle(cfg, sd, inp)
        assert torch.equal(ref["topk_proposals"].sort(1)[0], topk.sort(1)[0])
        f32 = figures(oracle(cfg, sd, inp, topk_proposals=topk), lib)
        assert max(f32.values()) < 1e-4, f32
        out[P + "seed"], out[P + "input_seed"] = np.array(c["seed"]), np.array(seed)
        out[P + "sd_keys"] = np.array(list(sd.keys()))
        for k, v in sd.items():
            out[P + "sum." + k] = checksum(v)
        out[P + "memory_q"] = (inp["memory"] * 8.0).round().to(torch.int8).numpy()
        out[P + "text_q"] = (inp["text"] * 8.0).round().to(torch.int8).numpy()
        rows, qs = pick(inp["memory"].shape[1], 48), pick(cfg["num_queries"], 24)
        out[P + "topk"], out[P + "rows_s"], out[P + "q_s"] = topk.numpy(), rows, qs
        out[P + "scores"] = lib["scores"][:, rows].numpy()
        out[P + "gap"], out[P + "invalid_selected"] = np.array(gap), np.array(int(torch.isinf(torch.gather(lib["prop"], 1, topk.unsqueeze(-1).repeat(1, 1, 4))).any()))
        out[P + "states"] = torch.stack(lib["states"])[:, :, qs].numpy()
        out[P + "references"] = torch.stack(lib["references"])[:, :, qs].numpy()
        out[P + "init_reference_points"] = lib["init_reference_points"].numpy()
        out[P + "logits"], out[P + "pred_boxes"] = torch.stack(lib["logits"]).numpy(), torch.stack(lib["pred_boxes"]).numpy()
        twin16 = None
        for dtype, tag in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
            tw = oracle(cfg, rounded(sd, dtype), inp, topk_proposals=topk, twin=dtype)
            fig = figures(tw, lib)
            for k, v in fig.items():
                out[P + f"twin.{tag}.{k}"] = np.array(v)
            out[P + f"twin.{tag}.scores_maxabs"] = np.array(float((tw["scores"] - lib["scores"]).abs().max()))
            if dtype == torch.float16:
                twin16 = fig
            print(f"  config {name} twin {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
        for dname in gd.DEFECTS:
            fig = figures(oracle(cfg, sd, inp, topk_proposals=topk, defect=dname), lib)
            eff = max(fig[k] / twin16[k] for k in ("pred_boxes", "last_state", "logits"))
            out[P + "defect." + dname] = np.array(eff)
            print(f"  config {name} defect {dname}: {eff:.1f} x the fp16 twin")
            if dname in NOT_APPLICABLE[name]:
                continue
            assert eff >= SENSITIVITY, f"condition 1: config {name}, defect {dname}: {eff:.2f} x the fp16 twin's figure"
    return out


def main():
    torch.manual_seed(0)
    out = build()
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
