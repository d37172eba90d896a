"""GroundingDINO's feature enhancer on the HIP kernels: the neck of ``transformers.GroundingDinoModel`` (``input_proj_vision``,
``level_embed``, ``text_projection``, the sine position embedding) and its ``GroundingDinoEncoder``, for inference — what stands between
:class:`omg_amd.SwinBackbone` (and the library's BERT) and the detector's decoder.

Parameters are kept under the library's own key names (``input_proj_vision.{l}.0 / .1``, ``level_embed``, ``text_projection``,
``encoder.layers.{i}.fusion_layer.*``, ``.text_enhancer_layer.*``, ``.deformable_layer.*``); ``load_state_dict(prefix="model.")`` takes
them out of a ``GroundingDinoForObjectDetection`` state dict and ignores its other keys.

  1x1 convolutions of the neck, every Linear   -> omg_gemm on NHWC rows: bias and the residual in its epilogue
  GroupNorm(32, 256) of the neck               -> omg_groupnorm_res_act
  the extra level (3x3, stride 2, padding 1)   -> omg_conv3x3_nhwc_act
  LayerNorms                                   -> omg_layernorm
  fusion (GroundingDinoBiMultiHeadAttention)   -> omg_attn_bi_vision + omg_attn_bi_text on the fused rows vision q | v and text k | v;
                                                  vision_param / text_param are folded into out_vision_proj / out_text_proj when the
                                                  operands are packed (product in fp32, rounded once); the residual is the
                                                  LayerNorm-ed features, as in the library
  text self-attention under the phrase mask    -> omg_attn_masked on the fused q | k rows of (h + pos) and the v rows of h
  multi-scale deformable attention             -> omg_msdeform_attn on the fused rows sampling_offsets | attention_weights of (h + pos)
                                                  and the value_proj rows of h (the padding mask zeroes VALUE rows)
  ReLU of the MLPs                             -> omg_relu, in place

Once per call, as torch ops on the device and outside the layer loop: the level masks (nearest interpolation of the pixel mask), the
sine position embedding + ``level_embed``, the valid ratios, the reference points, the text position embedding.  The library casts
``encode_sinusoidal_position_embedding(position_ids[..., None], 256)`` to the dtype of ``position_ids``; so does this module (integer
ids give an embedding truncated to integers).

Inference only: dropout and drop-path are the identity whatever the config says, ``train(True)`` is refused.  There is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib as L
from . import ops
from ._checkpoint import FlatWeights

__all__ = ["GroundingDinoEncoder", "GroundingDinoEncoderOutput", "check_config"]

_DROPS = ("dropout", "attention_dropout", "activation_dropout", "fusion_dropout", "fusion_droppath", "text_enhancer_dropout")


def _refuse(key: str, why: str):
    raise L.OmgHipError(f"GroundingDinoEncoder: config key '{key}': {why}")


def check_config(config) -> dict:
    """``GroundingDinoConfig`` / its dict -> the plain dict the module keeps.  Anything the kernels do not compute is refused with the
    key named."""
    cfg = dict(config.to_dict() if hasattr(config, "to_dict") else config)
    if cfg.get("d_model", 256) != 256:
        _refuse("d_model", f"{cfg['d_model']} has no kernel (the bi-attention is built for 4 heads of 256 on d_model 256)")
    if cfg.get("encoder_attention_heads", 8) != 8:
        _refuse("encoder_attention_heads", f"{cfg['encoder_attention_heads']} has no kernel (omg_msdeform_attn: head_dim 32; omg_attn_masked: 64)")
    if cfg.get("encoder_ffn_dim", 2048) != 2048:
        _refuse("encoder_ffn_dim", f"{cfg['encoder_ffn_dim']} has no kernel (the fusion's embed_dim is encoder_ffn_dim / 2 = 4 x 256)")
    if cfg.get("encoder_n_points", 4) != 4:
        _refuse("encoder_n_points", f"{cfg['encoder_n_points']} has no kernel (omg_msdeform_attn samples 4 points)")
    if not 1 <= cfg.get("num_feature_levels", 4) <= 4:
        _refuse("num_feature_levels", f"{cfg['num_feature_levels']} has no kernel (omg_msdeform_attn takes 1 to 4 levels)")
    if cfg.get("activation_function", "relu") != "relu":
        _refuse("activation_function", f"'{cfg['activation_function']}' has no kernel in these MLPs (omg_relu)")
    if cfg.get("position_embedding_type", "sine") != "sine":
        _refuse("position_embedding_type", f"'{cfg['position_embedding_type']}' is not built (sine only)")
    if cfg.get("max_text_len", 256) > 256:
        _refuse("max_text_len", f"{cfg['max_text_len']} is beyond the attention kernels (T at most 256)")
    text_hidden = cfg.get("text_hidden")
    if text_hidden is None:
        tc = cfg.get("text_config") or {}
        tc = tc.to_dict() if hasattr(tc, "to_dict") else tc
        text_hidden = tc.get("hidden_size", 768)
    in_channels = cfg.get("in_channels")
    if in_channels is None:
        bc = cfg.get("backbone_config") or {}
        bc = bc.to_dict() if hasattr(bc, "to_dict") else bc
        E, nst = bc.get("embed_dim", 96), len(bc.get("depths", [2, 2, 6, 2]))
        names = ["stem"] + [f"stage{i + 1}" for i in range(nst)]
        of, oi = bc.get("out_features"), bc.get("out_indices")
        if of is None:
            of = [names[i] for i in oi] if oi is not None else [names[-1]]
        in_channels = [E << (int(s[5:]) - 1) for s in of]
    in_channels = [int(c) for c in in_channels]
    Lv = int(cfg.get("num_feature_levels", 4))
    if len(in_channels) > Lv:
        _refuse("num_feature_levels", f"{Lv} levels for {len(in_channels)} backbone feature maps")
    for c in in_channels + [int(text_hidden)]:
        if c % 8 or c < 8:
            _refuse("backbone_config", f"a width of {c} into the neck; omg_gemm takes multiples of 8")
    return dict(d_model=256, heads=8, ffn=2048, points=4, levels=Lv, layers=int(cfg.get("encoder_layers", 6)),
                temperature=float(cfg.get("positional_embedding_temperature", 20)), eps=float(cfg.get("layer_norm_eps", 1e-5)),
                max_text_len=int(cfg.get("max_text_len", 256)), text_hidden=int(text_hidden), in_channels=in_channels)


class GroundingDinoEncoderOutput:
    def __init__(self, **kw):
        self.last_hidden_state_vision = kw.pop("last_hidden_state_vision")
        self.last_hidden_state_text = kw.pop("last_hidden_state_text")
        self.vision_hidden_states = kw.pop("vision_hidden_states", None)
        self.text_hidden_states = kw.pop("text_hidden_states", None)
        self.attentions = None
        for k, v in kw.items():        # spatial_shapes, spatial_shapes_list, level_start_index, valid_ratios, mask_flatten, vision_position_embedding, ...
            setattr(self, k, v)


def sine_position(mask: torch.Tensor, d_model: int, temperature: float) -> torch.Tensor:
    """GroundingDinoSinePositionEmbedding on a validity mask [B, H, W] -> [B, H W, d_model] fp32: normalised cumulative sums, scale
    2 pi, y before x."""
    nd = d_model // 2
    y = mask.cumsum(1, dtype=torch.float32)
    x = mask.cumsum(2, dtype=torch.float32)
    y = y / (y[:, -1:, :] + 1e-6) * (2 * math.pi)
    x = x / (x[:, :, -1:] + 1e-6) * (2 * math.pi)
    dim_t = torch.arange(nd, dtype=torch.float32, device=mask.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / nd)
    px, py = x[:, :, :, None] / dim_t, y[:, :, :, None] / dim_t
    px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), dim=4).flatten(3)
    py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), dim=4).flatten(3)
    return torch.cat((py, px), dim=3).flatten(1, 2)


def text_position(position_ids: torch.Tensor, d_model: int) -> torch.Tensor:
    """The library's encode_sinusoidal_position_embedding(position_ids[..., None], d_model), its cast to the ids' dtype included."""
    dim_t = torch.arange(d_model, dtype=torch.float32, device=position_ids.device)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / d_model)
    e = position_ids[..., None] * (2 * math.pi) / dim_t
    return torch.stack((e[..., 0::2].sin(), e[..., 1::2].cos()), dim=-1).flatten(-2).to(position_ids.dtype)


def reference_points(spatial: Sequence[Tuple[int, int]], valid_ratios: torch.Tensor) -> torch.Tensor:
    """GroundingDinoEncoder.get_reference_points: a query's point on its own level's grid and valid ratio, then times the valid ratio of
    every sampled level -> [B, N, L, 2] fp32 (x, y)."""
    refs = []
    for l, (h, w) in enumerate(spatial):
        ry, rx = torch.meshgrid(torch.linspace(0.5, h - 0.5, h, dtype=torch.float32, device=valid_ratios.device),
                                torch.linspace(0.5, w - 0.5, w, dtype=torch.float32, device=valid_ratios.device), indexing="ij")
        ry = ry.reshape(-1)[None] / (valid_ratios[:, None, l, 1] * h)
        rx = rx.reshape(-1)[None] / (valid_ratios[:, None, l, 0] * w)
        refs.append(torch.stack((rx, ry), -1))
    return (torch.cat(refs, 1)[:, :, None] * valid_ratios[:, None]).contiguous()


def _device_ints(rows, device) -> torch.Tensor:
    """A small int64 tensor of Python numbers, filled on the device (no host-to-device copy: legal under graph capture)."""
    t = torch.empty((len(rows),) + ((len(rows[0]),) if isinstance(rows[0], (tuple, list)) else ()), dtype=torch.long, device=device)
    for i, r in enumerate(rows):
        if isinstance(r, (tuple, list)):
            for j, x in enumerate(r):
                t[i, j].fill_(int(x))
        else:
            t[i].fill_(int(r))
    return t


class GroundingDinoEncoder(FlatWeights):
    """``GroundingDinoEncoder(config, dtype, device)``; ``config``: the library's ``GroundingDinoConfig`` or its dict.
    ``load_state_dict`` takes ``sd`` under the library's names; ``prefix="model."`` takes the neck and the encoder out of a
    ``GroundingDinoForObjectDetection`` state dict.  Keys outside the prefix, and the detector's other parts (backbone, text backbone,
    decoder, heads), are ignored; an ``input_proj_vision`` / ``encoder.`` key this config does not have is unexpected."""

    check_config = staticmethod(check_config)
    prefix = "model."
    no_training = ", ".join(repr(k) for k in _DROPS)

    # ------------------------------------------------------------------ parameters
    def shapes(self) -> Dict[str, tuple]:
        c = self.cfg
        d, ffn, H8, Lv, P = c["d_model"], c["ffn"], c["heads"], c["levels"], c["points"]
        E = ffn // 2
        out = {"level_embed": (Lv, d), "text_projection.weight": (d, c["text_hidden"]), "text_projection.bias": (d,)}
        cin = c["in_channels"]
        for l in range(Lv):
            k = 1 if l < len(cin) else 3
            ci = cin[l] if l < len(cin) else (cin[-1] if l == len(cin) else d)
            out[f"input_proj_vision.{l}.0.weight"], out[f"input_proj_vision.{l}.0.bias"] = (d, ci, k, k), (d,)
            out[f"input_proj_vision.{l}.1.weight"], out[f"input_proj_vision.{l}.1.bias"] = (d,), (d,)
        for i in range(c["layers"]):
            p = f"encoder.layers.{i}."
            f = p + "fusion_layer."
            out[f + "vision_param"], out[f + "text_param"] = (d,), (d,)
            for n in ("layer_norm_vision", "layer_norm_text"):
                out[f + n + ".weight"], out[f + n + ".bias"] = (d,), (d,)
            for n in ("vision_proj", "text_proj", "values_vision_proj", "values_text_proj"):
                out[f + f"attn.{n}.weight"], out[f + f"attn.{n}.bias"] = (E, d), (E,)
            for n in ("out_vision_proj", "out_text_proj"):
                out[f + f"attn.{n}.weight"], out[f + f"attn.{n}.bias"] = (d, E), (d,)
            t = p + "text_enhancer_layer."
            for n in ("query", "key", "value", "out_proj"):
                out[t + f"self_attn.{n}.weight"], out[t + f"self_attn.{n}.bias"] = (d, d), (d,)
            out[t + "fc1.weight"], out[t + "fc1.bias"], out[t + "fc2.weight"], out[t + "fc2.bias"] = (E, d), (E,), (d, E), (d,)
            for n in ("layer_norm_before", "layer_norm_after"):
                out[t + n + ".weight"], out[t + n + ".bias"] = (d,), (d,)
            m = p + "deformable_layer."
            out[m + "self_attn.sampling_offsets.weight"], out[m + "self_attn.sampling_offsets.bias"] = (H8 * Lv * P * 2, d), (H8 * Lv * P * 2,)
            out[m + "self_attn.attention_weights.weight"], out[m + "self_attn.attention_weights.bias"] = (H8 * Lv * P, d), (H8 * Lv * P,)
            for n in ("value_proj", "output_proj"):
                out[m + f"self_attn.{n}.weight"], out[m + f"self_attn.{n}.bias"] = (d, d), (d,)
            out[m + "fc1.weight"], out[m + "fc1.bias"], out[m + "fc2.weight"], out[m + "fc2.bias"] = (ffn, d), (ffn,), (d, ffn), (d,)
            for n in ("self_attn_layer_norm", "final_layer_norm"):
                out[m + n + ".weight"], out[m + n + ".bias"] = (d,), (d,)
        return out

    def _unexpected(self, k, ck):
        return ck if ck.startswith(("input_proj_vision.", "encoder.layers.", "level_embed", "text_projection.")) else None

    # ------------------------------------------------------------------ kernel operands that are not the checkpoint's own tensors, built once
    def _pack(self) -> dict:
        w, c = self._w, self.cfg
        cat = lambda names: torch.cat([w[n] for n in names], dim=0).contiguous()
        pk = {}
        for l in range(c["levels"]):
            k = f"input_proj_vision.{l}.0.weight"
            # 1x1: the GEMM weight [256, C]; 3x3: [Cout, 3, 3, Cin] for the NHWC convolution
            pk[k] = w[k].reshape(w[k].shape[0], -1).contiguous() if l < len(c["in_channels"]) else w[k].permute(0, 2, 3, 1).contiguous()
        for i in range(c["layers"]):
            p = f"encoder.layers.{i}."
            f, t, m = p + "fusion_layer.attn.", p + "text_enhancer_layer.self_attn.", p + "deformable_layer.self_attn."
            pk[f + "vis.weight"], pk[f + "vis.bias"] = cat([f + "vision_proj.weight", f + "values_vision_proj.weight"]), cat([f + "vision_proj.bias", f + "values_vision_proj.bias"])
            pk[f + "txt.weight"], pk[f + "txt.bias"] = cat([f + "text_proj.weight", f + "values_text_proj.weight"]), cat([f + "text_proj.bias", f + "values_text_proj.bias"])
            for side in ("vision", "text"):
                g = w[p + f"fusion_layer.{side}_param"].float()
                pk[f + f"out_{side}.weight"] = (g[:, None] * w[f + f"out_{side}_proj.weight"].float()).to(self._dtype).contiguous()
                pk[f + f"out_{side}.bias"] = (g * w[f + f"out_{side}_proj.bias"].float()).to(self._dtype).contiguous()
            pk[t + "qk.weight"], pk[t + "qk.bias"] = cat([t + "query.weight", t + "key.weight"]), cat([t + "query.bias", t + "key.bias"])
            pk[m + "ow.weight"] = cat([m + "sampling_offsets.weight", m + "attention_weights.weight"])
            pk[m + "ow.bias"] = cat([m + "sampling_offsets.bias", m + "attention_weights.bias"])
        return pk

    # ------------------------------------------------------------------ forward
    def _nhwc(self, fm: torch.Tensor) -> torch.Tensor:
        """An NCHW feature map as contiguous NHWC in the storage dtype: SwinBackbone's permuted NHWC views are taken without a copy."""
        x = fm.permute(0, 2, 3, 1)
        if x.dtype != self._dtype:
            x = x.to(self._dtype)
        return x if x.is_contiguous() else x.contiguous()

    @torch.no_grad()
    def forward(self, feature_maps: Sequence[torch.Tensor], pixel_mask: Optional[torch.Tensor], text_hidden_states: torch.Tensor,
                text_token_mask: torch.Tensor, text_self_attention_masks: torch.Tensor, position_ids: torch.Tensor,
                output_hidden_states: bool = False, **_ignored) -> GroundingDinoEncoderOutput:
        """``feature_maps``: NCHW, one per backbone level; ``pixel_mask`` [B, H, W] (1 = a real pixel) or None; ``text_hidden_states``
        [B, T, text_hidden] (the text backbone's last_hidden_state); ``text_token_mask`` [B, T] True = a real token;
        ``text_self_attention_masks`` [B, T, T] True = attend and ``position_ids`` [B, T], as
        generate_masks_with_special_tokens_and_transfer_map makes them."""
        c, w, dt = self.cfg, self._w, self._dtype
        fms = list(feature_maps)
        if not fms or not fms[0].is_cuda:
            raise L.OmgHipError("GroundingDinoEncoder needs its inputs on the MI355X (cuda/hip device); there is no CPU fallback")
        if len(fms) != len(c["in_channels"]) or any(f.dim() != 4 or f.shape[1] != ci for f, ci in zip(fms, c["in_channels"])):
            raise L.OmgHipError(f"GroundingDinoEncoder: feature maps {[tuple(f.shape) for f in fms]} are not NCHW with channels {c['in_channels']}")
        dev = fms[0].device
        B, T = fms[0].shape[0], text_hidden_states.shape[1]
        if T > c["max_text_len"] or T < 1:
            raise L.OmgHipError(f"GroundingDinoEncoder: {T} text tokens; 'max_text_len' is {c['max_text_len']}")
        d, eps, H8 = c["d_model"], c["eps"], c["heads"]
        pk = self._pk()

        # ---- the neck: 1x1 convolution + GroupNorm per level; extra levels by a 3x3 stride-2 convolution
        maps: List[torch.Tensor] = []                        # NHWC [B, h, w, 256]
        last_in = None
        for l in range(c["levels"]):
            P = f"input_proj_vision.{l}."
            if l < len(fms):
                x = self._nhwc(fms[l])
                last_in = x
                h_, w_ = x.shape[1], x.shape[2]
                y = ops.gemm(x.view(B * h_ * w_, x.shape[3]), pk[P + "0.weight"], bias=w[P + "0.bias"]).view(B, h_, w_, d)
            else:
                # the first extra level reads the backbone's LAST feature map, later ones the previous projected map
                y = ops.conv3x3_nhwc_act(last_in if l == len(fms) else maps[-1], pk[P + "0.weight"], stride=2, bias=w[P + "0.bias"])
            maps.append(ops.groupnorm_res_act(y, w[P + "1.weight"], w[P + "1.bias"], 32, 1e-5))
        spatial = [(m.shape[1], m.shape[2]) for m in maps]
        N = sum(h_ * w_ for h_, w_ in spatial)
        v = torch.cat([m.view(B, -1, d) for m in maps], dim=1).contiguous().view(B * N, d)

        # ---- once per call, torch on the device: masks, position embeddings, valid ratios, reference points
        has_mask = pixel_mask is not None
        if has_mask:
            masks = [F.interpolate(pixel_mask[None].float(), size=s).to(torch.bool)[0] for s in spatial]
        else:
            masks = [torch.ones((B,) + s, dtype=torch.bool, device=dev) for s in spatial]
        pos = torch.cat([sine_position(mk, d, c["temperature"]) + w["level_embed"][l].float().view(1, 1, -1)
                         for l, mk in enumerate(masks)], dim=1).to(dt).contiguous()
        mask_flatten = torch.cat([mk.flatten(1) for mk in masks], dim=1).contiguous()
        valid_ratios = torch.stack([torch.stack([mk[:, 0, :].sum(1).float() / mk.shape[2], mk[:, :, 0].sum(1).float() / mk.shape[1]], -1)
                                    for mk in masks], 1)
        ref = reference_points(spatial, valid_ratios)
        starts, s_ = [], 0
        for h_, w_ in spatial:
            starts.append(s_)
            s_ += h_ * w_
        vis_keep = mask_flatten.to(torch.uint8) if has_mask else None
        txt_keep = text_token_mask.to(device=dev, dtype=torch.bool).to(torch.uint8).contiguous()
        self_keep = text_self_attention_masks.to(device=dev, dtype=torch.bool).to(torch.uint8).contiguous()
        tpos = text_position(position_ids.to(dev), d).to(dt).contiguous().view(B * T, d)
        pos2 = pos.view(B * N, d)

        t = ops.gemm(text_hidden_states.to(dt).reshape(B * T, -1).contiguous(), w["text_projection.weight"], bias=w["text_projection.bias"])
        vs, ts = [v.view(B, N, d)], [t.view(B, T, d)]
        E = c["ffn"] // 2
        for i in range(c["layers"]):
            p = f"encoder.layers.{i}."
            # ---- fusion: the residual is the LayerNorm-ed features, on both sides
            f = p + "fusion_layer."
            vn = ops.layernorm(v, w[f + "layer_norm_vision.weight"], w[f + "layer_norm_vision.bias"], eps)
            tn = ops.layernorm(t, w[f + "layer_norm_text.weight"], w[f + "layer_norm_text.bias"], eps)
            vis = ops.gemm(vn, pk[f + "attn.vis.weight"], bias=pk[f + "attn.vis.bias"]).view(B, N, 2 * E)
            txt = ops.gemm(tn, pk[f + "attn.txt.weight"], bias=pk[f + "attn.txt.bias"]).view(B, T, 2 * E)
            ov = ops.attn_bi_vision(vis, txt, H8 // 2, 256 ** -0.5, text_mask=txt_keep)
            ot = ops.attn_bi_text(vis, txt, H8 // 2, 256 ** -0.5, vision_mask=vis_keep)
            v = ops.gemm(ov.view(B * N, E), pk[f + "attn.out_vision.weight"], bias=pk[f + "attn.out_vision.bias"], residual=vn)
            t = ops.gemm(ot.view(B * T, E), pk[f + "attn.out_text.weight"], bias=pk[f + "attn.out_text.bias"], residual=tn)
            # ---- text enhancer (post-norm): q = k = h + pos, v = h
            e = p + "text_enhancer_layer."
            tq = ops.add_(t.clone(), tpos)
            qk = ops.gemm(tq, pk[e + "self_attn.qk.weight"], bias=pk[e + "self_attn.qk.bias"]).view(B, T, 2 * d)
            tv = ops.gemm(t, w[e + "self_attn.value.weight"], bias=w[e + "self_attn.value.bias"]).view(B, T, d)
            o = ops.attn_masked(qk[..., :d], qk[..., d:], tv, H8 // 2, 64 ** -0.5, mask=self_keep)
            t = ops.gemm(o.view(B * T, d), w[e + "self_attn.out_proj.weight"], bias=w[e + "self_attn.out_proj.bias"], residual=t)
            t = ops.layernorm(t, w[e + "layer_norm_before.weight"], w[e + "layer_norm_before.bias"], eps)
            u = ops.gemm(t, w[e + "fc1.weight"], bias=w[e + "fc1.bias"])
            ops.relu(u, out=u)
            t = ops.gemm(u, w[e + "fc2.weight"], bias=w[e + "fc2.bias"], residual=t)
            t = ops.layernorm(t, w[e + "layer_norm_after.weight"], w[e + "layer_norm_after.bias"], eps)
            # ---- deformable layer (post-norm): offsets and logits from h + pos, the value from h
            m = p + "deformable_layer."
            hq = ops.add_(v.clone(), pos2)
            ow = ops.gemm(hq, pk[m + "self_attn.ow.weight"], bias=pk[m + "self_attn.ow.bias"])
            val = ops.gemm(v, w[m + "self_attn.value_proj.weight"], bias=w[m + "self_attn.value_proj.bias"])
            s = ops.msdeform_attn(val.view(B, N, d), ow.view(B, N, -1), ref, spatial, heads=H8, points=c["points"], mask=vis_keep, level_start=starts)
            v = ops.gemm(s.view(B * N, d), w[m + "self_attn.output_proj.weight"], bias=w[m + "self_attn.output_proj.bias"], residual=v)
            v = ops.layernorm(v, w[m + "self_attn_layer_norm.weight"], w[m + "self_attn_layer_norm.bias"], eps)
            u = ops.gemm(v, w[m + "fc1.weight"], bias=w[m + "fc1.bias"])
            ops.relu(u, out=u)
            v = ops.gemm(u, w[m + "fc2.weight"], bias=w[m + "fc2.bias"], residual=v)
            v = ops.layernorm(v, w[m + "final_layer_norm.weight"], w[m + "final_layer_norm.bias"], eps)
            vs.append(v.view(B, N, d))
            ts.append(t.view(B, T, d))
        return GroundingDinoEncoderOutput(
            last_hidden_state_vision=vs[-1], last_hidden_state_text=ts[-1],
            vision_hidden_states=tuple(vs) if output_hidden_states else None, text_hidden_states=tuple(ts) if output_hidden_states else None,
            spatial_shapes=_device_ints(spatial, dev), spatial_shapes_list=spatial,
            level_start_index=_device_ints(starts, dev), valid_ratios=valid_ratios, mask_flatten=mask_flatten,
            vision_position_embedding=pos, reference_points=ref, neck_maps=tuple(maps))
