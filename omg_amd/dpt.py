"""The DPT-hybrid depth estimator of the "Depth" spatial condition on the HIP kernels: ``transformers.DPTForDepthEstimation`` for the
architecture of ``Intel/dpt-hybrid-midas`` (the demos' default ``--dpt_checkpoint``), its image processor, and the tail of ``get_depth``.

The module tree and parameter names are those of the Hugging Face checkpoint (``dpt.embeddings.backbone.bit.*``, ``dpt.encoder.layer.{i}.*``,
``neck.*``, ``head.head.{0,2,4}``), so a ``dpt-hybrid-midas`` directory loads key for key.  NCHW pixel values in (fp32 or 16-bit),
``predicted_depth`` fp32 ``[B, H, W]`` out; NHWC 16-bit inside.

  BiT stem 7x7 / 2, TF-"SAME"               -> omg_dpt_stem_conv (packed dot products), weight standardisation folded at load in fp32
  GroupNorm (+ ReLU, + shortcut)            -> omg_groupnorm_res_act: the bottleneck's tail is one pass
  max-pool 3x3 / 2, SAME, pad value 0       -> omg_maxpool3x3s2_nhwc
  1x1 convolutions, every Linear            -> omg_gemm on the NHWC rows (a stride-2 shortcut reads a strided slice made contiguous)
  3x3 convolutions                          -> omg_conv3x3_nhwc_ex (SAME origin at stride 2; ReLU on load and in the epilogue for the
                                               pre-activation residual units) / omg_conv3x3_nhwc_act
  ViT: LayerNorm, QKV, attention, MLP       -> omg_layernorm, omg_gemm on the fused QKV weight, omg_attn_fwd (row-major V above 128
                                               keys, V^T below: ops.value_operand), omg_gelu_erf
  readout "project"                         -> omg_gemm of the tokens against the first half of the weight; the cls half is a
                                               per-sample bias (one small omg_gemm)
  bilinear x2 (align_corners=True)          -> omg_upsample2x_bilinear_nhwc
  head 32 -> 1 + ReLU, fp32                 -> omg_rowdot_f32
  get_depth's resize / normalise / 8-bit    -> omg_depth_tail (:func:`depth_condition`)

Everything else is refused with ``OmgHipError`` and the config key that caused it: plain ``dpt-large`` (``is_hybrid``), pre-activation
BiT layers, a readout other than ``project``, batch norm in the fusion units, ``add_projection``, an input that is not ``image_size``
(the position table is applied at its stored size; the fusion layers' residual resize never fires at an input that is a multiple of 32 and
is not built).  ``dpt.layernorm`` is held for a complete state dict and never applied: the depth path taps the hidden states in front
of it.  Inference only; there is no CPU path.
"""
from __future__ import annotations

import json
import math
import os
from types import SimpleNamespace
from typing import Dict, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._checkpoint import PackedCache, Weight as _W, param as _param, read_checkpoint

__all__ = ["DPTForDepthEstimation", "DPTImageProcessor", "DPTFeatureExtractor", "depth_condition", "check_config", "fold_weight_standardization"]

WS_EPS = 1e-8           # BiT's weight standardisation
GN_EPS = 1e-5           # BitGroupNormActivation


def fold_weight_standardization(w: torch.Tensor) -> torch.Tensor:
    """Per output channel ``(w - mean) / sqrt(biased var + 1e-8)`` in fp32: what BiT's convolutions compute on every call."""
    w = w.float()
    m = w.mean(dim=(1, 2, 3), keepdim=True)
    v = w.var(dim=(1, 2, 3), keepdim=True, unbiased=False)
    return (w - m) / torch.sqrt(v + WS_EPS)


# ------------------------------------------------------------------------------------------------ config
def _refuse(key: str, why: str):
    raise L.OmgHipError(f"DPTForDepthEstimation: config key '{key}': {why} (only the dpt-hybrid-midas architecture is built)")


def check_config(cfg: dict) -> dict:
    """The ``config.json`` of a checkpoint -> the few numbers the module needs; anything that is not dpt-hybrid-midas's architecture is
    refused with the key that says so."""
    g = cfg.get
    if not g("is_hybrid", False):
        _refuse("is_hybrid", "plain DPT (dpt-large: patch embedding, four reassemble layers) is not built")
    if g("readout_type", "project") != "project":
        _refuse("readout_type", f"'{g('readout_type')}' is not built, only 'project'")
    if g("use_batch_norm_in_fusion_residual", False):
        _refuse("use_batch_norm_in_fusion_residual", "batch norm in the fusion units is not built")
    if g("use_bias_in_fusion_residual", None) is False:
        _refuse("use_bias_in_fusion_residual", "fusion units without bias are not built")
    if g("add_projection", False):
        _refuse("add_projection", "the extra head projection is not built")
    if g("hidden_act", "gelu") != "gelu":
        _refuse("hidden_act", f"'{g('hidden_act')}' is not built, only 'gelu'")
    if not g("qkv_bias", True):
        _refuse("qkv_bias", "attention without bias is not built")
    if g("num_channels", 3) != 3:
        _refuse("num_channels", "the stem takes 3 channels")
    if list(g("neck_ignore_stages", [0, 1])) != [0, 1]:
        _refuse("neck_ignore_stages", "must be [0, 1]")
    if [float(f) for f in g("reassemble_factors", [1, 1, 1, 0.5])] != [1.0, 1.0, 1.0, 0.5]:
        _refuse("reassemble_factors", "must be [1, 1, 1, 0.5]")
    if g("head_in_index", -1) != -1:
        _refuse("head_in_index", "must be -1")
    b = dict(g("backbone_config") or {})
    if b.get("model_type", "bit") != "bit":
        _refuse("backbone_config.model_type", "the backbone must be BiT")
    if b.get("layer_type", "bottleneck") != "bottleneck":
        _refuse("backbone_config.layer_type", f"'{b.get('layer_type')}' is not built, only 'bottleneck'")
    if str(b.get("global_padding", "same")).lower() != "same":
        _refuse("backbone_config.global_padding", "must be 'same'")
    if not b.get("embedding_dynamic_padding", True):
        _refuse("backbone_config.embedding_dynamic_padding", "must be true")
    if b.get("hidden_act", "relu") != "relu":
        _refuse("backbone_config.hidden_act", "must be 'relu'")
    out = dict(image_size=g("image_size", 384), patch_size=g("patch_size", 16), hidden_size=g("hidden_size", 768),
               num_attention_heads=g("num_attention_heads", 12), num_hidden_layers=g("num_hidden_layers", 12),
               intermediate_size=g("intermediate_size", 3072), layer_norm_eps=g("layer_norm_eps", 1e-12),
               backbone_out_indices=list(g("backbone_out_indices", [2, 5, 8, 11])), neck_hidden_sizes=list(g("neck_hidden_sizes", [256, 512, 768, 768])),
               fusion_hidden_size=g("fusion_hidden_size", 256), backbone_featmap_shape=list(g("backbone_featmap_shape", [1, 1024, 24, 24])),
               bit=dict(depths=list(b.get("depths", [3, 4, 9])), hidden_sizes=list(b.get("hidden_sizes", [256, 512, 1024])),
                        embedding_size=b.get("embedding_size", 64), num_groups=b.get("num_groups", 32)))
    bit = out["bit"]
    if not isinstance(out["image_size"], int):
        _refuse("image_size", "must be one integer (square input)")
    if len(bit["depths"]) != 3 or len(bit["hidden_sizes"]) != 3:
        _refuse("backbone_config.depths", "three stages")
    if bit["embedding_size"] % 32 or bit["embedding_size"] > 128:
        _refuse("backbone_config.embedding_size", "a multiple of 32 up to 128 (omg_dpt_stem_conv)")
    if bit["num_groups"] > 64 or any((c // 4) % bit["num_groups"] or (c // 4) % 8 for c in bit["hidden_sizes"]) or bit["embedding_size"] % bit["num_groups"]:
        _refuse("backbone_config.num_groups", "at most 64 groups dividing every width; bottleneck widths multiples of 8")
    D, nh = out["hidden_size"], out["num_attention_heads"]
    if D % nh or D // nh != 64:
        _refuse("num_attention_heads", "heads of 64 (omg_attn_fwd)")
    if len(out["backbone_out_indices"]) != 4 or len(out["neck_hidden_sizes"]) != 4:
        _refuse("backbone_out_indices", "four taps")
    if any(not 0 <= i < out["num_hidden_layers"] for i in out["backbone_out_indices"][2:]):
        _refuse("backbone_out_indices", "taps beyond the encoder")
    S, P = out["image_size"], out["patch_size"]
    grid = S // P
    if S % 32 or math.ceil(S / 16) != grid or out["backbone_featmap_shape"][1:] != [bit["hidden_sizes"][2], grid, grid]:
        _refuse("backbone_featmap_shape", f"must be [1, {bit['hidden_sizes'][2]}, {grid}, {grid}]: the stage-3 map of a {S} x {S} input, one token per pixel")
    if out["neck_hidden_sizes"][:2] != bit["hidden_sizes"][:2] or any(c % 8 for c in out["neck_hidden_sizes"]) or out["fusion_hidden_size"] % 16:
        _refuse("neck_hidden_sizes", "the first two must be the widths of BiT's stages 1 and 2; all multiples of 8")
    return out


# ------------------------------------------------------------------------------------------------ the checkpoint's module tree
class _Holder(nn.Module):
    def __init__(self, **mods):
        super().__init__()
        for k, m in mods.items():
            self.add_module(k, m)


def _mlist(mods):
    return nn.ModuleList(list(mods))


def _bottleneck(cin, cout, first, dt, dev):
    mid = cout // 4
    mods = {}
    if first:
        mods["downsample"] = _Holder(conv=_W((cout, cin, 1, 1), 0, dt, dev), norm=_W((cout,), cout, dt, dev))
    mods.update(conv1=_W((mid, cin, 1, 1), 0, dt, dev), norm1=_W((mid,), mid, dt, dev), conv2=_W((mid, mid, 3, 3), 0, dt, dev),
                norm2=_W((mid,), mid, dt, dev), conv3=_W((cout, mid, 1, 1), 0, dt, dev), norm3=_W((cout,), cout, dt, dev))
    return _Holder(**mods)


def _vit_layer(D, I, dt, dev):
    lin = lambda o, i: _W((o, i), o, dt, dev)                                         # noqa: E731
    return _Holder(attention=_Holder(attention=_Holder(query=lin(D, D), key=lin(D, D), value=lin(D, D)), output=_Holder(dense=lin(D, D))),
                   intermediate=_Holder(dense=lin(I, D)), output=_Holder(dense=lin(D, I)),
                   layernorm_before=_W((D,), D, dt, dev), layernorm_after=_W((D,), D, dt, dev))


def _unit(c, dt, dev):
    return _Holder(convolution1=_W((c, c, 3, 3), c, dt, dev), convolution2=_W((c, c, 3, 3), c, dt, dev))


class DepthEstimatorOutput(SimpleNamespace):
    """``.predicted_depth`` (and ``.features`` when asked for)."""


class DPTForDepthEstimation(PackedCache):
    def __init__(self, config: dict, dtype=torch.float16, device=None):
        super().__init__()
        cfg = self.cfg = check_config(config)
        self.config = SimpleNamespace(**config)
        dt, dev = dtype, device
        bit = cfg["bit"]
        E, G = bit["embedding_size"], bit["num_groups"]
        chans = [E] + bit["hidden_sizes"]
        stages = _mlist(_Holder(layers=_mlist(_bottleneck(chans[s] if j == 0 else chans[s + 1], chans[s + 1], j == 0, dt, dev) for j in range(d)))
                        for s, d in enumerate(bit["depths"]))
        backbone = _Holder(bit=_Holder(embedder=_Holder(convolution=_W((E, 3, 7, 7), 0, dt, dev), norm=_W((E,), E, dt, dev)),
                                       encoder=_Holder(stages=stages)))
        D, I = cfg["hidden_size"], cfg["intermediate_size"]
        grid = cfg["image_size"] // cfg["patch_size"]
        emb = _Holder(backbone=backbone, projection=_W((D, cfg["backbone_featmap_shape"][1], 1, 1), D, dt, dev))
        emb.cls_token = _param((1, 1, D), dt, dev)
        emb.position_embeddings = _param((1, grid * grid + 1, D), dt, dev)
        self.dpt = _Holder(embeddings=emb, encoder=_Holder(layer=_mlist(_vit_layer(D, I, dt, dev) for _ in range(cfg["num_hidden_layers"]))),
                           layernorm=_W((D,), D, dt, dev))
        nhs, F = cfg["neck_hidden_sizes"], cfg["fusion_hidden_size"]
        re3 = _Holder(projection=_W((nhs[3], D, 1, 1), nhs[3], dt, dev), resize=_W((nhs[3], nhs[3], 3, 3), nhs[3], dt, dev))
        reassemble = _Holder(layers=_mlist([nn.Identity(), nn.Identity(), _Holder(projection=_W((nhs[2], D, 1, 1), nhs[2], dt, dev)), re3]),
                             readout_projects=_mlist([nn.Sequential(nn.Identity()), nn.Sequential(nn.Identity()),
                                                      nn.Sequential(_W((D, 2 * D), D, dt, dev)), nn.Sequential(_W((D, 2 * D), D, dt, dev))]))
        fusion = _Holder(layers=_mlist(_Holder(projection=_W((F, F, 1, 1), F, dt, dev), residual_layer1=_unit(F, dt, dev), residual_layer2=_unit(F, dt, dev))
                                       for _ in range(4)))
        self.neck = _Holder(reassemble_stage=reassemble, convs=_mlist(_W((F, c, 3, 3), 0, dt, dev) for c in nhs), fusion_stage=fusion)
        self.head = _Holder(head=_mlist([_W((F // 2, F, 3, 3), F // 2, dt, dev), nn.Identity(), _W((32, F // 2, 3, 3), 32, dt, dev), nn.Identity(),
                                         _W((1, 32, 1, 1), 1, dt, dev), nn.Identity()]))
        self.num_groups, self.grid = G, grid
        self._folded: Dict[str, torch.Tensor] = {}          # fp32 folds of the weight-standardised convolutions, from the checkpoint's own precision

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_pretrained(cls, path, torch_dtype=torch.float16, device=None, **_ignored):
        """A local checkpoint directory: ``config.json`` and ``model.safetensors`` or ``pytorch_model.bin``."""
        config, sd = read_checkpoint(path, "DPTForDepthEstimation")
        model = cls(config, dtype=torch_dtype, device=device)
        model.load_state_dict(sd, strict=True)
        return model.eval()

    def _ws_keys(self):
        return [k for k in self.state_dict() if ".backbone.bit." in k and k.endswith(".weight") and (".conv" in k or k.endswith("convolution.weight"))]

    def _load_from_state_dict(self, state_dict, prefix, *a, **k):
        """The folds are taken here, from the incoming tensors in their own precision, so that a load through a parent refolds too; they
        are kept on the weights' device, stay fp32 through ``.to()`` and follow a later move when they are packed."""
        dev = self.device
        self._folded = {key: fold_weight_standardization(state_dict[prefix + key]).to(dev) for key in self._ws_keys() if prefix + key in state_dict}
        return super()._load_from_state_dict(state_dict, prefix, *a, **k)

    @property
    def dtype(self):
        return self.dpt.layernorm.weight.dtype

    @property
    def device(self):
        return self.dpt.layernorm.weight.device

    # ------------------------------------------------------------------ kernel operands that are not the checkpoint's own tensors, built once
    def _pack(self) -> dict:
        dt, dev = self.dtype, self.device
        sd = dict(self.state_dict())
        pk: dict = {}

        def ws(key):                                       # folded in fp32 (from the checkpoint's tensor when it was loaded), rounded once
            f = self._folded.get(key)
            return (f if f is not None else fold_weight_standardization(sd[key])).to(device=dev, dtype=dt)

        def k33(w):
            return w.permute(0, 2, 3, 1).contiguous()

        def k11(w):
            return w.reshape(w.shape[0], -1).contiguous()

        P = "dpt.embeddings.backbone.bit."
        pk["stem"] = ops.pack_dpt_stem_weight(ws(P + "embedder.convolution.weight"))
        for key in self._ws_keys():
            if key.endswith("embedder.convolution.weight"):
                continue
            w = ws(key)
            pk[key] = k33(w) if w.shape[-1] == 3 else k11(w)
        e = self.dpt.embeddings
        pk["proj"] = k11(e.projection.weight.data)
        pos = e.position_embeddings.data[0]
        pk["cls_pos"] = (e.cls_token.data[0, 0].float() + pos[0].float()).to(dt)
        pk["pos_tok"] = pos[1:].contiguous()
        for i, ly in enumerate(self.dpt.encoder.layer):
            a = ly.attention.attention
            pk[f"qkv_w{i}"] = torch.cat([a.query.weight.data, a.key.weight.data, a.value.weight.data], dim=0).contiguous()
            pk[f"qkv_b{i}"] = torch.cat([a.query.bias.data, a.key.bias.data, a.value.bias.data], dim=0).contiguous()
        D = self.cfg["hidden_size"]
        rs = self.neck.reassemble_stage
        for i in (2, 3):
            w = rs.readout_projects[i][0].weight.data
            pk[f"ro_tok{i}"], pk[f"ro_cls{i}"] = w[:, :D].contiguous(), w[:, D:].contiguous()
            pk[f"re_proj{i}"] = k11(rs.layers[i].projection.weight.data)
        pk["re_resize"] = k33(rs.layers[3].resize.weight.data)
        for i, c in enumerate(self.neck.convs):
            pk[f"neck{i}"] = k33(c.weight.data)
        for i, ly in enumerate(self.neck.fusion_stage.layers):
            pk[f"fu_proj{i}"] = k11(ly.projection.weight.data)
            for u in ("residual_layer1", "residual_layer2"):
                for c in ("convolution1", "convolution2"):
                    pk[f"fu{i}.{u}.{c}"] = k33(getattr(getattr(ly, u), c).weight.data)
        h = self.head.head
        pk["head0"], pk["head2"], pk["head4"] = k33(h[0].weight.data), k33(h[2].weight.data), h[4].weight.data.reshape(-1).contiguous()
        return pk

    # ------------------------------------------------------------------ forward
    def _gn(self, m, x, relu=True, residual=None):
        return ops.groupnorm_res_act(x, m.weight.data, m.bias.data, self.num_groups, GN_EPS, residual=residual, relu=relu)

    @staticmethod
    def _conv1x1(x, w, bias=None):
        B, H, W, C = x.shape
        return ops.gemm(x.view(B * H * W, C), w, bias=bias).view(B, H, W, w.shape[0])

    def _unit(self, pk, name, m, x, add=None):
        """``x + conv2(relu(conv1(relu(x))))`` (+ ``add``): ReLU of x on load and of conv1 in its epilogue; the shortcut reads x as it is
        stored.  ``add`` is summed into x IN PLACE first (x is a neck convolution's output that nobody else reads)."""
        u = ops.conv3x3_nhwc_ex(x, pk[name + ".convolution1"], bias=m.convolution1.bias.data, act=2, relu_in=True)
        if add is not None:
            ops.add_(x, add)
        return ops.conv3x3_nhwc_ex(u, pk[name + ".convolution2"], bias=m.convolution2.bias.data, residual=x)

    @torch.no_grad()
    def forward_features(self, pixel_values: torch.Tensor) -> Dict[str, torch.Tensor]:
        """NCHW pixel values -> {"bit_stage1", "bit_stage2" (NHWC), "vit_tap0", "vit_tap1" ([B, N + 1, D]), "fused0" .. "fused3" (NHWC),
        "predicted_depth" (fp32 [B, H, W])}."""
        cfg, dt = self.cfg, self.dtype
        x = pixel_values
        if not x.is_cuda:
            raise L.OmgHipError("DPTForDepthEstimation needs its input on the MI355X (cuda/hip device); there is no CPU fallback")
        S = cfg["image_size"]
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, S, S):
            raise L.OmgHipError(f"DPTForDepthEstimation: input {tuple(x.shape)} is not [B, 3, {S}, {S}], the config's 'image_size' "
                                "(interpolating the position table is not built)")
        if x.dtype not in (torch.float32, dt):
            raise L.OmgHipError(f"DPTForDepthEstimation: pixel values must be float32 or {dt}, not {x.dtype}")
        B = x.shape[0]
        pk = self._pk()
        feats: Dict[str, torch.Tensor] = {}
        bit = self.dpt.embeddings.backbone.bit
        P = "dpt.embeddings.backbone.bit.encoder.stages."
        h = ops.dpt_stem_conv(x.contiguous(), pk["stem"])
        h = ops.maxpool3x3s2_nhwc(self._gn(bit.embedder.norm, h))
        maps = []
        for s, st in enumerate(bit.encoder.stages):
            for j, blk in enumerate(st.layers):
                stride = 2 if (s > 0 and j == 0) else 1
                key = f"{P}{s}.layers.{j}."
                sc = h
                if hasattr(blk, "downsample"):
                    xs = h[:, ::2, ::2].contiguous() if stride == 2 else h          # SAME at kernel 1, stride 2: no padding, every other pixel
                    sc = self._gn(blk.downsample.norm, self._conv1x1(xs, pk[key + "downsample.conv.weight"]), relu=False)
                t = self._gn(blk.norm1, self._conv1x1(h, pk[key + "conv1.weight"]))
                t = self._gn(blk.norm2, ops.conv3x3_nhwc_ex(t, pk[key + "conv2.weight"], stride=stride, same=True))
                h = self._gn(blk.norm3, self._conv1x1(t, pk[key + "conv3.weight"]), relu=True, residual=sc)
            maps.append(h)
        feats["bit_stage1"], feats["bit_stage2"] = maps[0], maps[1]

        # ---- ViT on the stage-3 map: one token per pixel, the cls token in front
        e = self.dpt.embeddings
        g, D, nh = self.grid, cfg["hidden_size"], cfg["num_attention_heads"]
        if tuple(maps[2].shape[1:3]) != (g, g):
            raise L.OmgHipError(f"DPTForDepthEstimation: stage-3 map {tuple(maps[2].shape)} against a {g} x {g} token grid ('backbone_featmap_shape')")
        N = g * g
        t = torch.empty((B, N + 1, D), dtype=dt, device=x.device)
        rows = maps[2].view(B, N, -1)
        for b in range(B):
            ops.gemm(rows[b], pk["proj"], bias=e.projection.bias.data, residual=pk["pos_tok"], out=t[b, 1:])
        t[:, 0] = pk["cls_pos"]
        t = t.view(B * (N + 1), D)
        eps = cfg["layer_norm_eps"]
        taps = []
        for i, ly in enumerate(self.dpt.encoder.layer):
            y = ops.layernorm(t, ly.layernorm_before.weight.data, ly.layernorm_before.bias.data, eps)
            qkv = ops.gemm(y, pk[f"qkv_w{i}"], bias=pk[f"qkv_b{i}"]).view(B, N + 1, 3 * D)
            o = ops.attention(qkv[:, :, :D], qkv[:, :, D:2 * D], ops.value_operand(qkv[:, :, 2 * D:], nh), nh, 1.0 / math.sqrt(D // nh))
            dense = ly.attention.output.dense
            t = ops.gemm(o.view(B * (N + 1), D), dense.weight.data, bias=dense.bias.data, residual=t)
            y = ops.layernorm(t, ly.layernorm_after.weight.data, ly.layernorm_after.bias.data, eps)
            u = ops.gemm(y, ly.intermediate.dense.weight.data, bias=ly.intermediate.dense.bias.data)
            ops.gelu_erf(u, out=u)
            t = ops.gemm(u, ly.output.dense.weight.data, bias=ly.output.dense.bias.data, residual=t)
            if i in cfg["backbone_out_indices"][2:]:
                taps.append(t.view(B, N + 1, D))
        feats["vit_tap0"], feats["vit_tap1"] = taps

        # ---- reassemble: readout "project" (the cls half of the Linear as a per-sample bias), 1x1 projection, stride-2 conv for the last
        rs = self.neck.reassemble_stage
        nmaps = [maps[0], maps[1]]
        for i, hs in zip((2, 3), taps):
            ro = rs.readout_projects[i][0]
            cls_bias = ops.gemm(hs[:, 0], pk[f"ro_cls{i}"], bias=ro.bias.data)                      # [B, D]
            z = torch.empty((B, N, D), dtype=dt, device=x.device)
            for b in range(B):
                ops.gemm(hs[b, 1:], pk[f"ro_tok{i}"], bias=cls_bias[b], out=z[b])
            ops.gelu_erf(z, out=z)
            pr = rs.layers[i].projection
            z = ops.gemm(z.view(B * N, D), pk[f"re_proj{i}"], bias=pr.bias.data).view(B, g, g, -1)
            if i == 3:
                z = ops.conv3x3_nhwc_act(z, pk["re_resize"], stride=2, bias=rs.layers[3].resize.bias.data)
            nmaps.append(z)
        nmaps = [ops.conv3x3_nhwc_act(m, pk[f"neck{i}"]) for i, m in enumerate(nmaps)]

        # ---- fusion, coarse to fine
        fused = None
        for i, (f, ly) in enumerate(zip(nmaps[::-1], self.neck.fusion_stage.layers)):
            if fused is None:
                fused = f
            else:
                if fused.shape != f.shape:
                    raise L.OmgHipError(f"DPTForDepthEstimation: fusion layer {i} gets {tuple(f.shape)} beside {tuple(fused.shape)}; "
                                        "the residual resize is not built ('image_size')")
                fused = self._unit(pk, f"fu{i}.residual_layer1", ly.residual_layer1, f, add=fused)
            fused = self._unit(pk, f"fu{i}.residual_layer2", ly.residual_layer2, fused)
            fused = self._conv1x1(ops.upsample2x_bilinear_nhwc(fused), pk[f"fu_proj{i}"], bias=ly.projection.bias.data)
            feats[f"fused{i}"] = fused

        # ---- head
        hd = self.head.head
        t = ops.upsample2x_bilinear_nhwc(ops.conv3x3_nhwc_act(fused, pk["head0"], bias=hd[0].bias.data))
        t = ops.conv3x3_nhwc_ex(t, pk["head2"], bias=hd[2].bias.data, act=2)
        Bh, Hh, Wh, _ = t.shape
        feats["predicted_depth"] = ops.rowdot_f32(t.view(Bh * Hh * Wh, 32), pk["head4"], hd[4].bias.data, relu=True).view(Bh, Hh, Wh)
        return feats

    def forward(self, pixel_values: torch.Tensor, **_ignored) -> DepthEstimatorOutput:
        return DepthEstimatorOutput(predicted_depth=self.forward_features(pixel_values)["predicted_depth"])


# ------------------------------------------------------------------------------------------------ the image processor (host side, PIL)
_RESAMPLE = {0: "NEAREST", 1: "LANCZOS", 2: "BILINEAR", 3: "BICUBIC", 4: "BOX", 5: "HAMMING"}


def _to_multiple(val, multiple):
    return int(round(val / multiple) * multiple)


class _Batch(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


class DPTImageProcessor:
    """``transformers.DPTImageProcessor`` for what a ``preprocessor_config.json`` carries: resize through PIL (``size``, ``resample``,
    ``keep_aspect_ratio``, ``ensure_multiple_of``), rescale, normalise.  Host side, fp32 NCHW out; padding is not built.  Cuda uint8
    [H, W, 3] tensors are prepared on the device instead (ops.image_prep), with the same bits, and ``pixel_values`` stays there."""

    def __init__(self, do_resize=True, size=None, resample=3, keep_aspect_ratio=False, ensure_multiple_of=1, do_rescale=True, rescale_factor=1 / 255,
                 do_normalize=True, image_mean=None, image_std=None, do_pad=False, **_ignored):
        size = size if size is not None else {"height": 384, "width": 384}
        if isinstance(size, int):
            size = {"height": size, "width": size}
        if do_pad:
            raise L.OmgHipError("DPTImageProcessor: config key 'do_pad': padding is not built")
        self.do_resize, self.size, self.resample = do_resize, {"height": int(size["height"]), "width": int(size["width"])}, int(resample)
        self.keep_aspect_ratio, self.ensure_multiple_of = bool(keep_aspect_ratio), int(ensure_multiple_of)
        self.do_rescale, self.rescale_factor, self.do_normalize = do_rescale, float(rescale_factor), do_normalize
        self.image_mean = [0.5, 0.5, 0.5] if image_mean is None else list(image_mean)
        self.image_std = [0.5, 0.5, 0.5] if image_std is None else list(image_std)

    @classmethod
    def from_pretrained(cls, path, **_ignored):
        f = os.path.join(os.fspath(path), "preprocessor_config.json")
        if not os.path.exists(f):
            raise L.OmgHipError(f"DPTImageProcessor.from_pretrained: no preprocessor_config.json in {path} (nothing is downloaded)")
        with open(f) as fh:
            return cls(**json.load(fh))

    def output_size(self, h: int, w: int) -> Tuple[int, int]:
        sh, sw = self.size["height"] / h, self.size["width"] / w
        if self.keep_aspect_ratio:                             # scale as little as possible
            if abs(1 - sw) < abs(1 - sh):
                sh = sw
            else:
                sw = sh
        return _to_multiple(sh * h, self.ensure_multiple_of), _to_multiple(sw * w, self.ensure_multiple_of)

    def _one(self, image) -> np.ndarray:
        from PIL import Image
        if isinstance(image, torch.Tensor):
            image = image.cpu().numpy()
        if isinstance(image, np.ndarray):
            if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
                raise L.OmgHipError("DPTImageProcessor takes PIL images or uint8 [H, W, 3] arrays")
            image = Image.fromarray(image)
        image = image.convert("RGB")
        if self.do_resize:
            oh, ow = self.output_size(image.height, image.width)
            image = image.resize((ow, oh), resample=getattr(Image, _RESAMPLE[self.resample]))
        a = np.asarray(image).astype(np.float32)
        if self.do_rescale:
            a = a * np.float32(self.rescale_factor)
        if self.do_normalize:
            a = (a - np.asarray(self.image_mean, dtype=np.float32)) / np.asarray(self.image_std, dtype=np.float32)
        return np.ascontiguousarray(a.transpose(2, 0, 1))

    def _one_device(self, image: torch.Tensor) -> torch.Tensor:
        """:meth:`_one` of a cuda uint8 [H, W, 3] tensor on the device -> fp32 [3, oh, ow]: Pillow's resize bit for bit and the numpy
        lines above as a lookup table (ops.image_prep)."""
        from . import image_prep
        image = image.contiguous()
        h, w = int(image.shape[0]), int(image.shape[1])
        oh, ow = self.output_size(h, w) if self.do_resize else (h, w)
        key = (image.device, self.do_rescale, self.rescale_factor, self.do_normalize, tuple(self.image_mean), tuple(self.image_std))
        if getattr(self, "_lut_key", None) != key:
            self._lut_key = key
            self._lut_t = image_prep.lut_numpy_rescale_mean_std(self.rescale_factor if self.do_rescale else None,
                                                                self.image_mean if self.do_normalize else None, self.image_std,
                                                                torch.float32, image.device)
        return ops.image_prep(image, (oh, ow), self.resample if self.do_resize else image_prep.BILINEAR, lut=self._lut_t)

    def __call__(self, images=None, return_tensors="pt", **_ignored):
        """PIL images and numpy arrays go through the host; cuda uint8 [H, W, 3] tensors stay on the device and ``pixel_values`` is there."""
        if images is None:
            raise L.OmgHipError("DPTImageProcessor: images=...")
        if return_tensors != "pt":
            raise L.OmgHipError("DPTImageProcessor: return_tensors must be 'pt'")
        if not isinstance(images, (list, tuple)):
            images = [images]
        on_device = [isinstance(im, torch.Tensor) and im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 for im in images]
        if images and all(on_device):
            return _Batch(pixel_values=torch.stack([self._one_device(im) for im in images]))
        return _Batch(pixel_values=torch.from_numpy(np.stack([self._one(im) for im in images])))

    preprocess = __call__


DPTFeatureExtractor = DPTImageProcessor


def depth_condition(estimator: DPTForDepthEstimation, processor: DPTImageProcessor, image, size: Sequence[int] = (1024, 1024)):
    """The demos' ``get_depth``: image -> the 8-bit three-channel depth condition (a PIL image of ``size`` = (height, width)), with the
    resize, the min-max normalisation and the quantisation on the device (omg_depth_tail).  A constant depth map gives a black image."""
    from PIL import Image
    x = processor(images=image, return_tensors="pt").pixel_values.to(estimator.device)
    depth = estimator(x).predicted_depth
    out = ops.depth_tail(depth, (int(size[0]), int(size[1])))
    return Image.fromarray(out[0].cpu().numpy())
