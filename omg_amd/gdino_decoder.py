"""GroundingDINO's query selection, decoder and heads on the HIP kernels: ``transformers.GroundingDinoModel.forward`` from "prepare
decoder inputs" on (``generate_encoder_output_proposals``, the two-stage top-k), ``GroundingDinoDecoder`` and the head loop of
``GroundingDinoForObjectDetection.forward``, for inference — what turns :class:`omg_amd.GroundingDinoEncoder`'s output into boxes.

Parameters are kept under the library's own key names (``enc_output``, ``enc_output_norm``, ``encoder_output_bbox_embed.layers.{j}``,
``query_position_embeddings.weight``, ``decoder.layers.{i}.*``, ``decoder.layer_norm``, ``decoder.reference_points_head.layers.{j}``,
``decoder.bbox_embed.{i}.layers.{j}``); ``load_state_dict(prefix="model.")`` takes them out of a ``GroundingDinoForObjectDetection``
state dict, which carries the box heads twice (``bbox_embed.*`` and ``model.decoder.bbox_embed.*``): either copy is taken, two copies
that differ are refused.

  every Linear                                  -> omg_gemm: bias and the residual in its epilogue
  LayerNorms                                    -> omg_layernorm
  the selection's score, the class head         -> omg_gdino_contrastive (row maximum only / padded fp32 logits)
  self-attention, text cross-attention          -> omg_attn_hd32 on the fused q | k rows of (h + pos) and the v rows of h; on the q rows
                                                   and the layer's k | v column slice of ONE text projection for all layers
  multi-scale deformable attention              -> omg_msdeform_attn_box on the fused rows sampling_offsets | attention_weights of
                                                   (h + pos) and the layer's column slice of ONE value_proj of the image memory
  logit / sigmoid / valid ratios / sine embed   -> omg_gdino_ref_step, once per layer (the box head's last Linear inside it)
  ReLU of the MLPs                              -> omg_relu, in place

Once per call, as torch ops on the device: the proposal grid, its validity test and inverse sigmoid, the zeroing of invalid and padded
memory rows, ``torch.topk`` / ``torch.gather`` (no host synchronisation: the call is capturable in a ``torch.cuda.graph``).  The box
MLP of ``encoder_output_bbox_embed`` runs on the selected rows only.

Inference only; ``output_attentions`` and the loss are not built.  There is no CPU path.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._checkpoint import FlatWeights, read_checkpoint

__all__ = ["GroundingDinoDecoderHead", "GroundingDinoDetectionOutput", "GroundingDinoDetector", "check_config", "detect", "phrases",
           "text_masks_from_input_ids", "SPECIAL_TOKENS"]

SPECIAL_TOKENS = (101, 102, 1012, 1029)          # [CLS], [SEP], '.', '?' of the BERT vocabulary


def _refuse(key: str, why: str):
    raise L.OmgHipError(f"GroundingDinoDecoderHead: config key '{key}': {why}")


def check_config(config) -> dict:
    """``GroundingDinoConfig`` / its dict -> the plain dict the module keeps.  Anything the kernels do not compute is refused with the
    key named."""
    cfg = dict(config.to_dict() if hasattr(config, "to_dict") else config)
    if not cfg.get("two_stage", True):
        _refuse("two_stage", "False is not built (the queries come from the encoder's proposals)")
    if not cfg.get("embedding_init_target", True):
        _refuse("embedding_init_target", "False is not built (the library itself fails there)")
    if cfg.get("query_dim", 4) != 4:
        _refuse("query_dim", f"{cfg['query_dim']} has no kernel (omg_msdeform_attn_box, omg_gdino_ref_step: 4 coordinates)")
    if cfg.get("d_model", 256) != 256:
        _refuse("d_model", f"{cfg['d_model']} has no kernel (omg_gdino_contrastive and omg_gdino_ref_step are built for 256 channels)")
    if cfg.get("decoder_attention_heads", 8) != 8:
        _refuse("decoder_attention_heads", f"{cfg['decoder_attention_heads']} has no kernel (omg_attn_hd32, omg_msdeform_attn_box: head_dim 32)")
    if cfg.get("decoder_n_points", 4) != 4:
        _refuse("decoder_n_points", f"{cfg['decoder_n_points']} has no kernel (omg_msdeform_attn_box samples 4 points)")
    ffn = cfg.get("decoder_ffn_dim", 2048)
    if ffn % 8 or ffn < 8:
        _refuse("decoder_ffn_dim", f"{ffn}: omg_gemm takes multiples of 8")
    if not 1 <= cfg.get("num_feature_levels", 4) <= 4:
        _refuse("num_feature_levels", f"{cfg['num_feature_levels']} has no kernel (omg_msdeform_attn_box takes 1 to 4 levels)")
    if cfg.get("activation_function", "relu") != "relu":
        _refuse("activation_function", f"'{cfg['activation_function']}' has no kernel in these MLPs (omg_relu)")
    mt = cfg.get("max_text_len", 256)
    if mt > 256 or mt % 4:
        _refuse("max_text_len", f"{mt} is beyond the kernels (omg_gdino_contrastive, omg_attn_hd32's text keys: a multiple of 4, at most 256)")
    return dict(d_model=256, heads=8, points=4, ffn=int(ffn), levels=int(cfg.get("num_feature_levels", 4)),
                layers=int(cfg.get("decoder_layers", 6)), num_queries=int(cfg.get("num_queries", 900)),
                eps=float(cfg.get("layer_norm_eps", 1e-5)), max_text_len=int(mt), share=bool(cfg.get("decoder_bbox_embed_share", True)))


class GroundingDinoDetectionOutput:
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def text_masks_from_input_ids(input_ids: torch.Tensor, special_token_ids: Sequence[int] = SPECIAL_TOKENS):
    """The library's generate_masks_with_special_tokens_and_transfer_map: the block self-attention mask [B, T, T] (tokens between two
    special tokens see each other and the closing one; everything sees itself) and the position ids [B, T] that restart behind every
    special token."""
    B, T = input_ids.shape
    dev = input_ids.device
    special = torch.zeros_like(input_ids, dtype=torch.bool)
    for s in special_token_ids:          # scalar compares, not torch.isin against a tensor made from the list: that is a host-to-device
        special = special | (input_ids == int(s))    # copy, which a torch.cuda.graph capture of the detector's call does not permit
    idx = torch.arange(T, device=dev)[None].expand(B, -1)
    prev = torch.cummax(torch.where(special, idx, torch.full((), -1, device=dev)), dim=1)[0]
    nxt = torch.where(special, idx, torch.full((), T, device=dev))
    nxt = torch.flip(torch.cummin(torch.flip(nxt, dims=[1]), dim=1)[0], dims=[1])
    valid = (nxt != 0) & (nxt != T - 1) & (nxt != T)
    mask = (nxt[:, :, None] == nxt[:, None, :]) & valid[:, None, :]
    mask = mask | torch.eye(T, device=dev, dtype=torch.bool)[None]
    pos = torch.where(valid, idx - prev - 1, torch.zeros_like(idx)).clamp(min=0).to(torch.long)
    return mask, pos


def proposals(mask_flatten: torch.Tensor, spatial: Sequence[Sequence[int]]):
    """generate_encoder_output_proposals without its Linear: mask_flatten [B, N] True = valid -> (proposal logits [B, N, 4] fp32 with
    +inf on padded and invalid rows, keep [B, N] True = the row's memory is not zeroed)."""
    B = mask_flatten.shape[0]
    dev = mask_flatten.device
    out, s = [], 0
    for level, (h, w) in enumerate(spatial):
        m = mask_flatten[:, s:s + h * w].view(B, h, w)
        vh, vw = m[:, :, 0].sum(1), m[:, 0, :].sum(1)
        gy, gx = torch.meshgrid(torch.linspace(0, h - 1, h, dtype=torch.float32, device=dev),
                                torch.linspace(0, w - 1, w, dtype=torch.float32, device=dev), indexing="ij")
        grid = torch.cat([gx.unsqueeze(-1), gy.unsqueeze(-1)], -1)
        scale = torch.cat([vw.unsqueeze(-1), vh.unsqueeze(-1)], 1).view(B, 1, 1, 2)
        grid = (grid.unsqueeze(0).expand(B, -1, -1, -1) + 0.5) / scale
        wh = torch.ones_like(grid) * 0.05 * (2.0 ** level)
        out.append(torch.cat((grid, wh), -1).view(B, -1, 4))
        s += h * w
    p = torch.cat(out, 1)
    ok = ((p > 0.01) & (p < 0.99)).all(-1)
    keep = ok & mask_flatten
    logit = torch.log(p / (1 - p)).masked_fill(~keep[..., None], float("inf"))
    return logit.contiguous(), keep


class GroundingDinoDecoderHead(FlatWeights):
    """``GroundingDinoDecoderHead(config, dtype, device)``; ``config``: the library's ``GroundingDinoConfig`` or its dict."""

    check_config = staticmethod(check_config)
    prefix = "model."
    no_training = "'dropout', 'attention_dropout', 'activation_dropout', the loss"

    # ------------------------------------------------------------------ parameters
    def shapes(self) -> Dict[str, tuple]:
        c = self.cfg
        d, ffn, H8, Lv, P = c["d_model"], c["ffn"], c["heads"], c["levels"], c["points"]
        out = {"query_position_embeddings.weight": (c["num_queries"], d)}

        def lin(name, o, i):
            out[name + ".weight"], out[name + ".bias"] = (o, i), (o,)

        def norm(name):
            out[name + ".weight"], out[name + ".bias"] = (d,), (d,)

        def mlp(name, i, o):
            lin(name + ".layers.0", d, i)
            lin(name + ".layers.1", d, d) if o is None else lin(name + ".layers.1", o, d)
            if o is None:
                lin(name + ".layers.2", 4, d)

        lin("enc_output", d, d)
        norm("enc_output_norm")
        mlp("encoder_output_bbox_embed", d, None)
        mlp("decoder.reference_points_head", 2 * d, d)
        norm("decoder.layer_norm")
        for i in range(c["layers"]):
            p = f"decoder.layers.{i}."
            for a in ("self_attn", "encoder_attn_text"):
                for n in ("query", "key", "value", "out_proj"):
                    lin(p + f"{a}.{n}", d, d)
            lin(p + "encoder_attn.sampling_offsets", H8 * Lv * P * 2, d)
            lin(p + "encoder_attn.attention_weights", H8 * Lv * P, d)
            lin(p + "encoder_attn.value_proj", d, d)
            lin(p + "encoder_attn.output_proj", d, d)
            for n in ("self_attn_layer_norm", "encoder_attn_text_layer_norm", "encoder_attn_layer_norm", "final_layer_norm"):
                norm(p + n)
            lin(p + "fc1", ffn, d)
            lin(p + "fc2", d, ffn)
            mlp(f"decoder.bbox_embed.{i}", d, None)
        return out

    def load_state_dict(self, sd, strict: bool = True, prefix: str = ""):
        """``sd`` under the library's names; ``prefix="model."`` takes this module's keys out of a ``GroundingDinoForObjectDetection``
        state dict and ignores the others.  The box heads are looked for under ``{prefix}decoder.bbox_embed.*`` and under the detection
        model's own ``bbox_embed.*``; where both are there they must be equal."""
        shapes, sd = self.shapes(), dict(sd)
        for top in [k for k in sd if k.startswith("bbox_embed.") and "decoder." + k in shapes]:
            mine = prefix + "decoder." + top
            if mine not in sd:
                sd[mine] = sd[top]
            elif not torch.equal(sd[mine].detach().cpu(), sd[top].detach().cpu()):
                raise L.OmgHipError(f"GroundingDinoDecoderHead.load_state_dict: {mine} and {top} differ; the library ties them")
        return super().load_state_dict(sd, strict, prefix)

    def _unexpected(self, k, ck):
        return k if ck.startswith(("enc_output", "encoder_output_bbox_embed.", "query_position_embeddings.", "decoder.")) else None

    # ------------------------------------------------------------------ kernel operands that are not the checkpoint's own tensors, built once
    def _pack(self) -> dict:
        w, c = self._w, self.cfg
        cat = lambda names: torch.cat([w[n] for n in names], dim=0).contiguous()
        lay = [f"decoder.layers.{i}." for i in range(c["layers"])]
        pk = {}
        for s in ("weight", "bias"):
            # constant over the layers: one GEMM of the image memory for every layer's value_proj, one of the text for every k | v
            pk["value_all." + s] = cat([p + "encoder_attn.value_proj." + s for p in lay])
            pk["text_kv_all." + s] = cat([p + f"encoder_attn_text.{n}." + s for p in lay for n in ("key", "value")])
            for p in lay:
                pk[p + "self_attn.qk." + s] = cat([p + "self_attn.query." + s, p + "self_attn.key." + s])
                pk[p + "encoder_attn.ow." + s] = cat([p + "encoder_attn.sampling_offsets." + s, p + "encoder_attn.attention_weights." + s])
        return pk

    # ------------------------------------------------------------------ forward
    def _lin(self, x, name, residual=None, relu=False):
        y = ops.gemm(x, self._w[name + ".weight"], bias=self._w[name + ".bias"], residual=residual)
        return ops.relu(y, out=y) if relu else y

    def _ln(self, x, name):
        return ops.layernorm(x, self._w[name + ".weight"], self._w[name + ".bias"], self.cfg["eps"])

    def _box_hidden(self, x, name):
        """The two hidden Linears of a box head; its last Linear runs inside omg_gdino_ref_step."""
        return self._lin(self._lin(x, name + ".layers.0", relu=True), name + ".layers.1", relu=True)

    @torch.no_grad()
    def forward(self, encoder_output, text_token_mask: torch.Tensor, output_hidden_states: bool = False,
                topk_proposals: Optional[torch.Tensor] = None) -> GroundingDinoDetectionOutput:
        """``encoder_output``: :class:`omg_amd.GroundingDinoEncoder`'s output object; ``text_token_mask`` [B, T] True = a real token;
        ``topk_proposals`` [B, num_queries] int64 replaces the selection."""
        c, w, dt = self.cfg, self._w, self._dtype
        mem, txt = encoder_output.last_hidden_state_vision, encoder_output.last_hidden_state_text
        if not mem.is_cuda:
            raise L.OmgHipError("GroundingDinoDecoderHead needs its inputs on the MI355X (cuda/hip device); there is no CPU fallback")
        dev = mem.device
        B, N, d = mem.shape
        T, Q, H8, NL = txt.shape[1], c["num_queries"], c["heads"], c["layers"]
        spatial = [(int(h_), int(w_)) for h_, w_ in encoder_output.spatial_shapes_list]
        if len(spatial) != c["levels"] or sum(h_ * w_ for h_, w_ in spatial) != N:
            raise L.OmgHipError(f"GroundingDinoDecoderHead: levels {spatial} do not make {N} rows on 'num_feature_levels' {c['levels']}")
        if not 1 <= T <= c["max_text_len"]:
            raise L.OmgHipError(f"GroundingDinoDecoderHead: {T} text tokens; 'max_text_len' is {c['max_text_len']}")
        if N < Q:
            raise L.OmgHipError(f"GroundingDinoDecoderHead: {N} image tokens for 'num_queries' {Q}")
        starts, s_ = [], 0
        for h_, w_ in spatial:
            starts.append(s_)
            s_ += h_ * w_
        pk = self._pk()
        mask_flatten = encoder_output.mask_flatten.to(device=dev, dtype=torch.bool)
        vis_keep = mask_flatten.to(torch.uint8).contiguous()
        txt_keep = text_token_mask.to(device=dev, dtype=torch.bool).to(torch.uint8).contiguous()
        vr = encoder_output.valid_ratios.to(device=dev, dtype=torch.float32).contiguous()
        mem = mem.to(dt).contiguous()
        txt = txt.to(dt).contiguous()
        mem2, txt2 = mem.view(B * N, d), txt.view(B * T, d)

        # ---- proposals and the selection: invalid rows keep the library's behaviour (query LayerNorm(bias), box logit +inf)
        prop, keep = proposals(mask_flatten, spatial)
        oq = self._ln(self._lin((mem * keep[..., None].to(dt)).view(B * N, d), "enc_output"), "enc_output_norm").view(B, N, d)
        if topk_proposals is None:
            score = ops.gdino_contrastive(oq, txt, txt_keep, c["max_text_len"], logits=False, rowmax=True)
            topk_proposals = torch.topk(score, Q, dim=1)[1]
        topk_proposals = topk_proposals.to(dev)
        sel = torch.gather(oq, 1, topk_proposals[..., None].expand(-1, -1, d)).contiguous()
        sel_logit = torch.gather(prop, 1, topk_proposals[..., None].expand(-1, -1, 4)).contiguous()
        hb = self._box_hidden(sel.view(B * Q, d), "encoder_output_bbox_embed").view(B, Q, d)
        e3 = "encoder_output_bbox_embed.layers.2."
        ref, ref_input, emb = ops.gdino_ref_step(vr, logit_in=sel_logit, hidden=hb, w3=w[e3 + "weight"], b3=w[e3 + "bias"])
        init_ref = ref

        # ---- constant over the layers
        value_all = ops.gemm(mem2, pk["value_all.weight"], bias=pk["value_all.bias"]).view(B, N, NL * d)
        text_kv = ops.gemm(txt2, pk["text_kv_all.weight"], bias=pk["text_kv_all.bias"]).view(B, T, NL * 2 * d)

        h = w["query_position_embeddings.weight"][None].expand(B, -1, -1).reshape(B * Q, d).contiguous()
        inter: List[torch.Tensor] = []
        refs: List[torch.Tensor] = []
        for i in range(NL):
            p = f"decoder.layers.{i}."
            pos = self._lin(self._lin(emb.view(B * Q, 2 * d), "decoder.reference_points_head.layers.0", relu=True), "decoder.reference_points_head.layers.1")
            # ---- self-attention: q = k = h + pos, v = h
            hq = ops.add_(h.clone(), pos)
            qk = ops.gemm(hq, pk[p + "self_attn.qk.weight"], bias=pk[p + "self_attn.qk.bias"]).view(B, Q, 2 * d)
            v = self._lin(h, p + "self_attn.value").view(B, Q, d)
            o = ops.attn_hd32(qk[..., :d], qk[..., d:], v, H8, 32 ** -0.5)
            h = self._ln(self._lin(o.view(B * Q, d), p + "self_attn.out_proj", residual=h), p + "self_attn_layer_norm")
            # ---- text cross-attention under the padded-token mask
            hq = ops.add_(h.clone(), pos)
            q = self._lin(hq, p + "encoder_attn_text.query").view(B, Q, d)
            o = ops.attn_hd32(q, text_kv[..., 2 * d * i:2 * d * i + d], text_kv[..., 2 * d * i + d:2 * d * (i + 1)], H8, 32 ** -0.5, key_mask=txt_keep)
            h = self._ln(self._lin(o.view(B * Q, d), p + "encoder_attn_text.out_proj", residual=h), p + "encoder_attn_text_layer_norm")
            # ---- deformable cross-attention at the box references
            hq = ops.add_(h.clone(), pos)
            ow = ops.gemm(hq, pk[p + "encoder_attn.ow.weight"], bias=pk[p + "encoder_attn.ow.bias"]).view(B, Q, -1)
            s = ops.msdeform_attn_box(value_all[..., d * i:d * (i + 1)], ow, ref_input, spatial, heads=H8, points=c["points"], mask=vis_keep,
                                      level_start=starts)
            h = self._ln(self._lin(s.view(B * Q, d), p + "encoder_attn.output_proj", residual=h), p + "encoder_attn_layer_norm")
            # ---- feed-forward
            h = self._ln(self._lin(self._lin(h, p + "fc1", relu=True), p + "fc2", residual=h), p + "final_layer_norm")
            # ---- the decoder's own refinement: the box head on the state BEFORE decoder.layer_norm
            b3 = f"decoder.bbox_embed.{i}.layers.2."
            hb = self._box_hidden(h, f"decoder.bbox_embed.{i}").view(B, Q, d)
            ref, ref_input, emb = ops.gdino_ref_step(vr, ref_in=ref, hidden=hb, w3=w[b3 + "weight"], b3=w[b3 + "bias"], embed=i + 1 < NL)
            inter.append(self._ln(h, "decoder.layer_norm").view(B, Q, d))
            refs.append(ref)

        # ---- the detection heads: the box head on the NORMED state plus the logit of the PREVIOUS level's reference
        levels = range(NL) if output_hidden_states else [NL - 1]
        all_logits, all_boxes = [], []
        for l in levels:
            b3 = f"decoder.bbox_embed.{l}.layers.2."
            hb = self._box_hidden(inter[l].view(B * Q, d), f"decoder.bbox_embed.{l}").view(B, Q, d)
            box, _, _ = ops.gdino_ref_step(vr, ref_in=init_ref if l == 0 else refs[l - 1], hidden=hb, w3=w[b3 + "weight"], b3=w[b3 + "bias"], embed=False)
            all_boxes.append(box)
            all_logits.append(ops.gdino_contrastive(inter[l], txt, txt_keep, c["max_text_len"]))
        return GroundingDinoDetectionOutput(
            logits=all_logits[-1], pred_boxes=all_boxes[-1], init_reference_points=init_ref, last_hidden_state=inter[-1],
            intermediate_hidden_states=torch.stack(inter, 1), intermediate_reference_points=torch.stack(refs, 1),
            topk_proposals=topk_proposals, all_logits=tuple(all_logits) if output_hidden_states else None,
            all_pred_boxes=tuple(all_boxes) if output_hidden_states else None)


# ------------------------------------------------------------------ front ends
def detect(outputs, box_threshold: float = 0.3, text_threshold: float = 0.25):
    """What the original package's ``predict`` computes before it decodes phrases, per sample: ``scores = sigmoid(logits).max(-1)``, the
    boxes with ``scores > box_threshold`` (cxcywh, normalised), their scores and per kept box the token mask ``sigmoid(logits) >
    text_threshold`` -> a list of (boxes [K, 4], scores [K], token_masks [K, max_text_len])."""
    prob = outputs.logits.sigmoid()
    scores = prob.max(-1)[0]
    out = []
    for b in range(prob.shape[0]):
        keep = scores[b] > box_threshold
        out.append((outputs.pred_boxes[b][keep], scores[b][keep], prob[b][keep] > text_threshold))
    return out


def phrases(token_masks: torch.Tensor, input_ids: torch.Tensor, tokenizer, special_token_ids: Sequence[int] = SPECIAL_TOKENS) -> List[str]:
    """Per kept box the phrase its token mask selects: the ids of one sample ``input_ids`` [T] at the selected positions, special tokens
    left out, through ``tokenizer.decode`` (host side)."""
    ids = input_ids.tolist()
    out = []
    for row in token_masks.tolist():
        out.append(tokenizer.decode([t for t, m in zip(ids, row[:len(ids)]) if m and t not in special_token_ids]))
    return out


class GroundingDinoDetector(nn.Module):
    """``SwinBackbone`` -> a caller-supplied text module -> ``GroundingDinoEncoder`` -> ``GroundingDinoDecoderHead``.  The text module
    is any callable ``(input_ids, attention_mask [B, T, T], token_type_ids, position_ids) -> last_hidden_state``: the library's BERT
    in torch, or :class:`omg_amd.BertTextEncoder` on the HIP kernels (``from_pretrained(..., text_backbone="hip")``)."""

    def __init__(self, backbone, text_backbone, encoder, head):
        super().__init__()
        self.backbone, self.text_backbone, self.encoder, self.head = backbone, text_backbone, encoder, head

    @classmethod
    def from_pretrained(cls, path, torch_dtype=torch.float16, device=None, text_backbone: str = "torch", **_ignored):
        """``text_backbone="torch"``: the library's BERT in torch, in fp32 (``torch_dtype`` does not apply to it); ``"hip"``:
        :class:`omg_amd.BertTextEncoder` in ``torch_dtype`` — every network of the call then runs on the HIP kernels and the call is
        capturable in one ``torch.cuda.graph``."""
        from .gdino import GroundingDinoEncoder
        from .swin import SwinBackbone
        if text_backbone not in ("torch", "hip"):
            raise L.OmgHipError(f"GroundingDinoDetector.from_pretrained: text_backbone='{text_backbone}'; 'torch' or 'hip'")
        config, sd = read_checkpoint(path, "GroundingDinoDetector")          # read once: the four parts are built from this pair
        backbone = SwinBackbone.from_state_dict(config, sd, torch_dtype=torch_dtype, device=device, prefix="model.backbone.conv_encoder.model.")
        encoder = GroundingDinoEncoder.from_state_dict(config, sd, torch_dtype=torch_dtype, device=device)
        head = GroundingDinoDecoderHead.from_state_dict(config, sd, torch_dtype=torch_dtype, device=device)
        if text_backbone == "hip":
            from .bert import BertTextEncoder
            return cls(backbone, BertTextEncoder.from_state_dict(config, sd, torch_dtype=torch_dtype, device=device), encoder, head)
        from transformers import AutoConfig, AutoModel
        tc = dict(config.get("text_config") or {})
        text = AutoModel.from_config(AutoConfig.for_model(tc.pop("model_type", "bert"), **tc), add_pooling_layer=False)
        pre = "model.text_backbone."
        text.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=False)
        text = text.to(device=device).eval()

        def text_backbone(input_ids, attention_mask, token_type_ids, position_ids):
            # the library hands its BERT the block mask as [B, 1, T, T]
            return text(input_ids=input_ids, attention_mask=attention_mask[:, None], token_type_ids=token_type_ids, position_ids=position_ids)[0]

        return cls(backbone, text_backbone, encoder, head)

    @torch.no_grad()
    def forward(self, pixel_values, input_ids, token_type_ids=None, attention_mask=None, pixel_mask=None):
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        self_mask, position_ids = text_masks_from_input_ids(input_ids)
        text = self.text_backbone(input_ids, self_mask, token_type_ids, position_ids)
        fms = self.backbone(pixel_values)
        fms = fms.feature_maps if hasattr(fms, "feature_maps") else fms
        token_mask = attention_mask.bool()
        enc = self.encoder(fms, pixel_mask, text, token_mask, self_mask, position_ids)
        return self.head(enc, token_mask)
