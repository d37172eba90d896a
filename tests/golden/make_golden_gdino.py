"""Generate tests/golden/gdino_golden.npz: what transformers' GroundingDinoModel neck modules (input_proj_vision, level_embed,
text_projection, its sine position embedding) and GroundingDinoEncoder compute in fp32 on the CPU for two small configs at the
enhancer's real widths (d_model 256, 8 heads, FFN 2048, 4 levels, 4 points), with two encoder layers.

    python tests/golden/make_golden_gdino.py        (from the repository root; CPU only, well under a minute)

The weights are NOT stored: tests/gdino_torch.py's ``seed_state`` regenerates them from the recorded seed and the per-key checksums pin
that.  Two configs (``gdino_torch.small_cfg``), under the prefixes ``a.`` and ``b.``:

    a   feature maps 64 / 128 / 256 channels on 13 x 19, 7 x 10, 4 x 5 (the extra level 2 x 3, N = 343), B = 2, sample 1's pixel mask
        pads its right and bottom; T = 11, three phrases, two padded tokens in sample 0
    b   9 x 25, 5 x 13, 3 x 7 (extra level 2 x 4, N = 319), no pixel mask; T = 37, one phrase of 30 tokens

Stored per config:
  cfg_seed, cfg_input_seed              the seeds (sizes and masks are gdino_torch.small_cfg / seeded_inputs)
  sd_keys, sum.<key>                    the state-dict keys and a float64 checksum per key
  fm<l>_q, text_q                       the inputs as int8: value = q / 8
  pixel_mask, text_token_mask, text_self_attention_masks, position_ids
  idx.vision, vision<i>                 the vision state before layer i (i = 0: the neck's output) .. after the last, at the rows idx.vision
  idx.text, text<i>                     the same for the text states
  twin_err.vision / .text               rms error / rms of gdino_torch's fp16 and bf16 twins on the last states
  defect.<name>.vision / .text          what each deliberate defect of gdino_torch.DEFECTS does to the last states (rms / rms)

SENSITIVITY.  Before the file is written the oracle is run, on the file's own inputs, with each defect, and each must move the last
vision OR text state by at least 10 x the fp16 twin's figure for that state.  That is a condition on the fixture (seeds and weight
scales), not a tolerance of any test."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import gdino_torch as gt  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gdino_golden.npz")
CONFIGS = {"a": dict(seed=51, input_seed=11), "b": dict(seed=52, input_seed=12)}
SENSITIVITY = 10.0


def pick(n, k):
    return np.unique(np.round(np.linspace(0, n - 1, min(n, k))).astype(np.int64))


def checksum(v: torch.Tensor) -> np.ndarray:
    return np.array(float((v.double() * torch.arange(1, v.numel() + 1, dtype=torch.float64).reshape(v.shape).remainder(7.0).add(1.0)).sum()))


def library_model(cfg):
    """A GroundingDinoModel whose backbone gives the config's channel counts (Swin, embed 32 -> 64 / 128 / 256): only its neck modules
    and its encoder are used."""
    from transformers import BertConfig, GroundingDinoConfig, SwinConfig
    from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoModel
    bc = SwinConfig(embed_dim=cfg["in_channels"][0] // 2, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8], window_size=7, out_indices=[2, 3, 4])
    tc = BertConfig(hidden_size=cfg["text_hidden"], num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, vocab_size=64)
    hc = GroundingDinoConfig(backbone_config=bc, text_config=tc, encoder_layers=cfg["encoder_layers"], decoder_layers=1, num_queries=8,
                             d_model=cfg["d_model"], encoder_attention_heads=cfg["encoder_attention_heads"], encoder_ffn_dim=cfg["encoder_ffn_dim"],
                             encoder_n_points=cfg["encoder_n_points"], num_feature_levels=cfg["num_feature_levels"],
                             positional_embedding_temperature=cfg["positional_embedding_temperature"], layer_norm_eps=cfg["layer_norm_eps"],
                             max_text_len=cfg["max_text_len"])
    return GroundingDinoModel(hc).eval(), hc


def library_run(cfg, sd, inp):
    """The library's own modules, composed as GroundingDinoModel.forward composes them.  -> (vision states, text states, neck maps)."""
    m, _ = library_model(cfg)
    own = m.state_dict()
    assert all(k in own and tuple(own[k].shape) == tuple(v.shape) for k, v in sd.items()), [k for k in sd if k not in own]
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith(("backbone.", "text_backbone.", "decoder.", "enc_output", "encoder_output", "query_position"))
                                  for k in missing), missing
    fms, pixel_mask = inp["feature_maps"], inp["pixel_mask"]
    B = fms[0].shape[0]
    if pixel_mask is None:
        pixel_mask = torch.ones((B,) + tuple(cfg["image"]), dtype=torch.long)
    with torch.no_grad():
        text = m.text_projection(inp["text_hidden_states"])
        maps, masks, poss = [], [], []
        for l in range(cfg["num_feature_levels"]):
            if l < len(fms):
                src = m.input_proj_vision[l](fms[l])
            else:
                src = m.input_proj_vision[l](fms[-1] if l == len(fms) else maps[-1])
            mask = torch.nn.functional.interpolate(pixel_mask[None].float(), size=src.shape[-2:]).to(torch.bool)[0]
            maps.append(src)
            masks.append(mask)
            poss.append(m.backbone.position_embedding(src, mask).to(src.dtype))
        sf, mf, pf, spatial = [], [], [], []
        for l, (src, mask, pe) in enumerate(zip(maps, masks, poss)):
            spatial.append(tuple(src.shape[-2:]))
            sf.append(src.flatten(2).transpose(1, 2))
            mf.append(mask.flatten(1))
            pf.append(pe.flatten(2).transpose(1, 2) + m.level_embed[l].view(1, 1, -1))
        sf, mf, pf = torch.cat(sf, 1), torch.cat(mf, 1), torch.cat(pf, 1)
        sp = torch.as_tensor(spatial, dtype=torch.long)
        lsi = torch.cat((sp.new_zeros((1,)), sp.prod(1).cumsum(0)[:-1]))
        vr = torch.stack([m.get_valid_ratio(mk) for mk in masks], 1).float()
        o = m.encoder(vision_features=sf, vision_attention_mask=~mf, vision_position_embedding=pf, spatial_shapes=sp,
                      spatial_shapes_list=spatial, level_start_index=lsi, valid_ratios=vr, text_features=text,
                      text_attention_mask=~inp["text_token_mask"], text_position_embedding=None,
                      text_self_attention_masks=~inp["text_self_attention_masks"], text_position_ids=inp["position_ids"],
                      output_hidden_states=True, return_dict=True)
    return o.vision_hidden_states, o.text_hidden_states, maps


def oracle(cfg, sd, inp, **kw):
    with torch.no_grad():
        return gt.forward(sd, cfg, inp["feature_maps"], inp["pixel_mask"], inp["text_hidden_states"], inp["text_token_mask"],
                          inp["text_self_attention_masks"], inp["position_ids"], **kw)


def build():
    out = {}
    for name, c in CONFIGS.items():
        P = name + "."
        cfg = gt.small_cfg(name)
        sd = gt.seed_state(cfg, c["seed"])
        inp = gt.seeded_inputs(cfg, c["input_seed"])
        out[P + "cfg_seed"], out[P + "cfg_input_seed"] = np.array(c["seed"]), np.array(c["input_seed"])
        out[P + "sd_keys"] = np.array(list(sd))
        for k, v in sd.items():
            out[P + "sum." + k] = checksum(v)
        for l, f in enumerate(inp["feature_maps"]):
            out[P + f"fm{l}_q"] = (f * 8.0).round().clamp(-127, 127).to(torch.int8).numpy()
        out[P + "text_q"] = (inp["text_hidden_states"] * 8.0).round().clamp(-127, 127).to(torch.int8).numpy()
        out[P + "pixel_mask"] = np.zeros(0, np.uint8) if inp["pixel_mask"] is None else inp["pixel_mask"].to(torch.uint8).numpy()
        for k in ("text_token_mask", "text_self_attention_masks"):
            out[P + k] = inp[k].to(torch.uint8).numpy()
        out[P + "position_ids"] = inp["position_ids"].numpy()
        vs, ts, _ = library_run(cfg, sd, inp)
        assert len(vs) == cfg["encoder_layers"] + 1
        iv, it = pick(vs[0].shape[1], 24), pick(ts[0].shape[1], 16)
        out[P + "idx.vision"], out[P + "idx.text"] = iv, it
        for i, (v, t) in enumerate(zip(vs, ts)):
            out[P + f"vision{i}"], out[P + f"text{i}"] = v[:, torch.from_numpy(iv)].numpy(), t[:, torch.from_numpy(it)].numpy()
        ref = oracle(cfg, sd, inp)
        rv, rt = ref["vision_states"][-1], ref["text_states"][-1]
        assert gt.rel_rms(rv, vs[-1]) < 1e-4 and gt.rel_rms(rt, ts[-1]) < 1e-4, (gt.rel_rms(rv, vs[-1]), gt.rel_rms(rt, ts[-1]))
        tw = {}
        for dt in (torch.float16, torch.bfloat16):
            sdr = {k: v.to(dt).float() for k, v in sd.items()}
            o = oracle(cfg, sdr, inp, twin=dt)
            tw[dt] = (gt.rel_rms(o["vision_states"][-1], rv), gt.rel_rms(o["text_states"][-1], rt))
        out[P + "twin_err.vision"] = np.array([tw[torch.float16][0], tw[torch.bfloat16][0]])
        out[P + "twin_err.text"] = np.array([tw[torch.float16][1], tw[torch.bfloat16][1]])
        for d in gt.DEFECTS:
            o = oracle(cfg, sd, inp, defect=d)
            dv, dtx = gt.rel_rms(o["vision_states"][-1], rv), gt.rel_rms(o["text_states"][-1], rt)
            out[P + f"defect.{d}.vision"], out[P + f"defect.{d}.text"] = np.array(dv), np.array(dtx)
            print(f"{name} {d:22s} vision {dv:.4f} ({dv / tw[torch.float16][0]:.0f} x twin)  text {dtx:.4f} ({dtx / tw[torch.float16][1]:.0f} x twin)")
            applies = not (d in ("no_value_mask", "valid_ratio_one", "no_vision_key_mask") and inp["pixel_mask"] is None)
            applies = applies and not (d == "no_text_key_mask" and bool(inp["text_token_mask"].all()))
            if applies:
                assert dv >= SENSITIVITY * tw[torch.float16][0] or dtx >= SENSITIVITY * tw[torch.float16][1], \
                    f"config {name}: the fixture does not see defect '{d}'"
            else:
                assert dv == 0.0 and dtx == 0.0, f"config {name}: defect '{d}' should not apply without the mask"
        print(f"{name} twins: fp16 {tw[torch.float16]}, bf16 {tw[torch.bfloat16]}")
    return out


def main():
    torch.manual_seed(0)
    out = build()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
