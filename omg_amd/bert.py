"""GroundingDINO's BERT text encoder on the HIP kernels: ``transformers``' ``BertModel(add_pooling_layer=False)`` for inference, under the
library's state-dict keys (``embeddings.*``, ``encoder.layer.{i}.attention.self.{query,key,value}``, ``.attention.output.{dense,LayerNorm}``,
``.intermediate.dense``, ``.output.{dense,LayerNorm}``).  ``pooler.*`` and ``embeddings.position_ids`` are accepted and dropped.

  the three embeddings and their LayerNorm   -> omg_bert_embed_ln, one launch, the int64 ids read on the device
  q | k | v                                  -> ONE Linear on the weights packed at load
  attention under the phrase block mask      -> omg_attn_masked on column slices of the fused rows, scale 1/8
  attention.output.dense, output.dense       -> a Linear with the residual in its epilogue, then omg_layernorm
  intermediate.dense                         -> a Linear with the erf GELU in its epilogue

Seven launches a layer and no elementwise pass.  A Linear is omg_gemm_skinny when ``T <= t_skinny`` and omg_gemm otherwise: a caption is
a handful of tokens, so M = B T is 6 to 30 rows against a 768- or 3072-wide weight — a weight stream, for which omg_gemm's 128 x 128
tiles leave all but a few compute units idle.  The choice is a function of T alone, never of B T: a caption gives the same bits alone
and inside a batch.  ``linear="skinny" | "gemm"`` forces either; on omg_gemm, which has no plain GELU epilogue, the intermediate
projection is followed by omg_gelu_erf (an eighth launch).

``forward(input_ids, attention_mask [B, T, T], token_type_ids, position_ids) -> last_hidden_state [B, T, hidden]`` is the callable
:class:`omg_amd.GroundingDinoDetector` documents for its text part, with the mask and the position ids of ``text_masks_from_input_ids``.
No step synchronises with the host: the call is capturable in a ``torch.cuda.graph``.  Inference only; there is no CPU path.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib as L
from . import ops
from ._checkpoint import FlatWeights

__all__ = ["BertTextEncoder", "check_config", "T_SKINNY"]

# The largest measured T up to which omg_gemm_skinny is no slower than omg_gemm on the sum of a layer's four Linears
# (tools/bert_bench.py, batch 1; both kernels on cache-resident weights).  It started at 64; profiles/bert_bench.log: "a layer's four
# Linears at T = 256: round 1: skinny 64.46 us, omg_gemm 95.95 us; round 2: skinny 64.39 us, omg_gemm 96.23 us; skinny is not slower in both
# rounds", and so at every smaller T of the list (T = 4: 17.6 us against 90.2 us) — the largest T the attention kernel takes, so "auto" is
# omg_gemm_skinny at every T a call can have at batch 1.  The rule stays a function of T: a batch of long captions (B T in the thousands)
# is where omg_gemm's tiles fill the chip; omg_gemm is reached through linear="gemm" or a smaller t_skinny.
T_SKINNY = 256
MAX_T = 256                       # omg_attn_masked


def _refuse(key: str, why: str):
    raise L.OmgHipError(f"BertTextEncoder: config key '{key}': {why}")


def check_config(config) -> dict:
    """``BertConfig`` / its dict -> the plain dict the module keeps.  Anything the kernels do not compute is refused with the key named."""
    cfg = dict(config.to_dict() if hasattr(config, "to_dict") else config)
    hidden, heads = int(cfg.get("hidden_size", 768)), int(cfg.get("num_attention_heads", 12))
    inter = int(cfg.get("intermediate_size", 3072))
    if hidden % 8 or hidden < 8 or hidden > 2048:
        _refuse("hidden_size", f"{hidden}: the kernels take multiples of 8 up to 2048 (omg_layernorm)")
    if heads < 1 or hidden != heads * 64:
        _refuse("num_attention_heads", f"{heads} heads on 'hidden_size' {hidden} is head_dim {hidden / max(heads, 1):g}; omg_attn_masked is built for 64")
    if inter % 8 or inter < 8:
        _refuse("intermediate_size", f"{inter}: omg_gemm and omg_gemm_skinny take multiples of 8")
    if cfg.get("hidden_act", "gelu") != "gelu":
        _refuse("hidden_act", f"'{cfg['hidden_act']}' has no epilogue (the erf GELU of gelu.h)")
    if cfg.get("position_embedding_type", "absolute") != "absolute":
        _refuse("position_embedding_type", f"'{cfg['position_embedding_type']}' is not built (absolute position rows only)")
    if cfg.get("is_decoder", False):
        _refuse("is_decoder", "True is not built (no causal mask, no cache)")
    if cfg.get("add_cross_attention", False):
        _refuse("add_cross_attention", "True is not built")
    return dict(hidden=hidden, heads=heads, inter=inter, layers=int(cfg.get("num_hidden_layers", 12)),
                vocab=int(cfg.get("vocab_size", 30522)), positions=int(cfg.get("max_position_embeddings", 512)),
                types=int(cfg.get("type_vocab_size", 2)), eps=float(cfg.get("layer_norm_eps", 1e-12)))


class BertTextEncoder(FlatWeights):
    """``BertTextEncoder(config, dtype, device, linear="auto")``; ``config``: the library's ``BertConfig`` or its dict.
    ``load_state_dict`` takes ``sd`` under the library's names; ``prefix="model.text_backbone."`` takes this module's keys out of a
    ``GroundingDinoForObjectDetection`` state dict and ignores the others.  ``pooler.*`` and ``embeddings.position_ids`` are dropped.
    ``from_pretrained`` takes a checkpoint directory of a ``GroundingDinoForObjectDetection`` (the config's ``text_config``, the keys under
    ``prefix``) or of a plain BERT (the top level of the config; pass the file's own prefix, ``""`` or ``"bert."``); ``linear`` and
    ``t_skinny`` go to the constructor."""

    check_config = staticmethod(check_config)
    prefix = "model.text_backbone."
    no_training = "'hidden_dropout_prob', 'attention_probs_dropout_prob'"
    constructor_keywords = ("linear", "t_skinny")

    def __init__(self, config, dtype=torch.float16, device=None, linear: str = "auto", t_skinny: int = T_SKINNY):
        super().__init__(config, dtype, device)
        if linear not in ("auto", "skinny", "gemm"):
            raise L.OmgHipError(f"BertTextEncoder: linear='{linear}'; 'auto', 'skinny' or 'gemm'")
        self.linear, self.t_skinny = linear, int(t_skinny)

    # ------------------------------------------------------------------ parameters
    def shapes(self) -> Dict[str, tuple]:
        c = self.cfg
        d, f = c["hidden"], c["inter"]
        out = {"embeddings.word_embeddings.weight": (c["vocab"], d), "embeddings.position_embeddings.weight": (c["positions"], d),
               "embeddings.token_type_embeddings.weight": (c["types"], d)}

        def lin(name, o, i):
            out[name + ".weight"], out[name + ".bias"] = (o, i), (o,)

        def norm(name):
            out[name + ".weight"], out[name + ".bias"] = (d,), (d,)

        norm("embeddings.LayerNorm")
        for i in range(c["layers"]):
            p = f"encoder.layer.{i}."
            for n in ("query", "key", "value"):
                lin(p + "attention.self." + n, d, d)
            lin(p + "attention.output.dense", d, d)
            norm(p + "attention.output.LayerNorm")
            lin(p + "intermediate.dense", f, d)
            lin(p + "output.dense", d, f)
            norm(p + "output.LayerNorm")
        return out

    @staticmethod
    def canonical_key(k: str, prefix: str = "") -> Optional[str]:
        k = FlatWeights.canonical_key(k, prefix)
        return None if k is None or k.startswith(("pooler.", "embeddings.position_ids")) else k

    @classmethod
    def from_state_dict(cls, config, sd, **keywords):
        return super().from_state_dict(config.get("text_config") or config, sd, **keywords)

    # ------------------------------------------------------------------ kernel operands that are not the checkpoint's own tensors, built once
    def _pack(self) -> dict:
        w = self._w
        pk = {}
        for i in range(self.cfg["layers"]):
            p = f"encoder.layer.{i}.attention.self."
            for s in ("weight", "bias"):
                pk[p + "qkv." + s] = torch.cat([w[p + n + "." + s] for n in ("query", "key", "value")], dim=0).contiguous()
        return pk

    # ------------------------------------------------------------------ forward
    def uses_skinny(self, T: int) -> bool:
        """Which kernel a Linear of a call with T tokens a sample runs on: a function of T alone."""
        return self.linear == "skinny" or (self.linear == "auto" and T <= self.t_skinny)

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, token_type_ids=None, position_ids=None, output_hidden_states: bool = False):
        """``input_ids`` [B, T] int64; ``attention_mask`` [B, T, T] (or [B, 1, T, T]) True / non-zero = attend, None = everything;
        ``token_type_ids`` / ``position_ids`` [B, T] int64, None = zeros / 0 .. T - 1.  -> last_hidden_state [B, T, hidden];
        ``output_hidden_states``: -> (last_hidden_state, (the embeddings' output, the state after every layer))."""
        c, w = self.cfg, self._w
        if self.training:
            raise L.OmgHipError("BertTextEncoder: training is not built; the module is inference only")
        B, T = input_ids.shape
        if T > MAX_T:
            _refuse("max_position_embeddings", f"{T} tokens; omg_attn_masked takes at most {MAX_T}")
        if T > c["positions"]:
            _refuse("max_position_embeddings", f"{T} tokens; the position table has {c['positions']} rows")
        if not input_ids.is_cuda or w["embeddings.word_embeddings.weight"].device != input_ids.device:
            raise L.OmgHipError("BertTextEncoder needs its inputs and weights on the MI355X (cuda/hip device); there is no CPU fallback")
        dev, d, H = input_ids.device, c["hidden"], c["heads"]
        input_ids = input_ids.to(torch.int64).contiguous()
        token_type_ids = torch.zeros_like(input_ids) if token_type_ids is None else token_type_ids.to(device=dev, dtype=torch.int64).contiguous()
        if position_ids is None:
            position_ids = torch.arange(T, device=dev, dtype=torch.int64)[None].expand(B, -1)
        position_ids = position_ids.to(device=dev, dtype=torch.int64).expand(B, T).contiguous()
        if attention_mask is not None:
            if attention_mask.dim() == 4:
                attention_mask = attention_mask[:, 0]
            if attention_mask.shape != (B, T, T):
                raise L.OmgHipError(f"BertTextEncoder: attention_mask is {tuple(attention_mask.shape)}; [B, T, T] = {(B, T, T)}")
            attention_mask = attention_mask.to(device=dev).ne(0).to(torch.uint8).contiguous()
        pk = self._pk()
        skinny = self.uses_skinny(T)

        def lin(x, weight, bias, residual=None, gelu=False):
            if skinny:
                return ops.gemm_skinny(x, weight, bias=bias, gelu=gelu, residual=residual)
            y = ops.gemm(x, weight, bias=bias, residual=residual)
            return ops.gelu_erf(y, out=y) if gelu else y

        e = "embeddings."
        h = ops.bert_embed_ln(input_ids, token_type_ids, position_ids, w[e + "word_embeddings.weight"], w[e + "token_type_embeddings.weight"],
                              w[e + "position_embeddings.weight"], w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], c["eps"]).view(B * T, d)
        states = [h]
        for i in range(c["layers"]):
            p = f"encoder.layer.{i}."
            qkv = lin(h, pk[p + "attention.self.qkv.weight"], pk[p + "attention.self.qkv.bias"]).view(B, T, 3 * d)
            o = ops.attn_masked(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], H, 0.125, mask=attention_mask).view(B * T, d)
            a = lin(o, w[p + "attention.output.dense.weight"], w[p + "attention.output.dense.bias"], residual=h)
            h = ops.layernorm(a, w[p + "attention.output.LayerNorm.weight"], w[p + "attention.output.LayerNorm.bias"], c["eps"])
            f = lin(h, w[p + "intermediate.dense.weight"], w[p + "intermediate.dense.bias"], gelu=True)
            a = lin(f, w[p + "output.dense.weight"], w[p + "output.dense.bias"], residual=h)
            h = ops.layernorm(a, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], c["eps"])
            states.append(h)
        if output_hidden_states:
            return h.view(B, T, d), tuple(s.view(B, T, d) for s in states)
        return h.view(B, T, d)
