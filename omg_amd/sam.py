"""SAM's prompt encoder, mask decoder and predictor on the HIP kernels: from the encoder's embedding and a box to a mask.

The module tree and parameter names are those of the ``segment_anything`` checkpoint layout that ``efficientvit_sam_*.pt`` files carry,
so ``prompt_encoder.*`` and ``mask_decoder.*`` load key for key beside ``image_encoder.*`` (omg_amd/efficientvit.py).  The predictor
reproduces ``EfficientViTSamPredictor`` of the reference (src/efficientvit/models/efficientvit/sam.py:244-460).

  Linear layers (q / k / v / out projections, MLPs, hypernetworks, IoU head)  -> omg_gemm (bias and the residual in its epilogue)
  attention at head_dim 32 (tokens) and 16 (both cross-attentions)            -> omg_attn_small on column slices of projection buffers
  LayerNorm                                                                   -> omg_layernorm
  ReLU of the MLPs                                                            -> omg_relu
  output_upscaling                                                            -> omg_gemm + omg_convt2x2_ln_gelu, twice
  masks = hypernetwork rows x upscaled embedding, only the rows that are returned -> omg_sam_mask_logits (fp32)
  postprocess_masks and the threshold                                         -> omg_sam_postprocess

The prompt encoder (a handful of Fourier features per call) is plain torch on the device, in fp32.  NHWC rows inside: the image
embedding is the encoder's ``"out"``.  Every GEMM runs per prompt, so a prompt's result does not depend on what else is in the batch.
Inference only; there is no CPU path, and a mask prompt is refused.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from . import efficientvit as _ev
from ._checkpoint import PackedCache, Seq as _Seq, Weight as _Weight
from .efficientvit import EfficientViTSamConfig, EfficientViTSamImageEncoder
from .litemla import LiteMLA

__all__ = ["SamPromptEncoder", "SamMaskDecoder", "EfficientViTSam", "EfficientViTSamPredictor", "efficientvit_sam", "efficientvit_sam_xl0",
           "efficientvit_sam_xl1", "create_sam_model", "set_norm_eps", "EfficientViTSamConfig", "EfficientViTSamImageEncoder"]


# ---------------------------------------------------------------------------------------------- prompt encoder
class _PositionEmbeddingRandom(nn.Module):
    def __init__(self, num_pos_feats, device):
        super().__init__()
        self.register_buffer("positional_encoding_gaussian_matrix", torch.randn(2, num_pos_feats, device=device))

    def encode(self, coords01: torch.Tensor) -> torch.Tensor:
        """(x, y) in [0, 1]^2 -> [..., 2 * num_pos_feats] fp32."""
        c = (2 * coords01.float() - 1) @ self.positional_encoding_gaussian_matrix.float()
        c = 2 * math.pi * c
        return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)


class SamPromptEncoder(PackedCache):
    def __init__(self, embed_dim: int = 256, image_embedding_size: Tuple[int, int] = (64, 64), input_image_size: Tuple[int, int] = (1024, 1024),
                 mask_in_chans: int = 16, dtype=torch.float16, device=None):
        super().__init__()
        self.embed_dim, self.image_embedding_size, self.input_image_size = embed_dim, tuple(image_embedding_size), tuple(input_image_size)
        self.pe_layer = _PositionEmbeddingRandom(embed_dim // 2, device)
        self.point_embeddings = nn.ModuleList([_Weight((1, embed_dim), 0, dtype, device) for _ in range(4)])
        self.not_a_point_embed = _Weight((1, embed_dim), 0, dtype, device)
        m = mask_in_chans
        # held so that the state dict is complete; a mask prompt is refused
        self.mask_downscaling = _Seq({0: _Weight((m // 4, 1, 2, 2), m // 4, dtype, device), 1: _Weight((m // 4,), m // 4, dtype, device),
                                      3: _Weight((m, m // 4, 2, 2), m, dtype, device), 4: _Weight((m,), m, dtype, device),
                                      6: _Weight((embed_dim, m, 1, 1), embed_dim, dtype, device)})
        self.no_mask_embed = _Weight((1, embed_dim), 0, dtype, device)

    @property
    def dtype(self):
        return self.no_mask_embed.weight.dtype

    def get_dense_pe(self) -> torch.Tensor:
        """The positional encoding of the embedding grid as NHWC rows [H * W, embed_dim] in the storage dtype; computed once."""
        g = self.pe_layer.positional_encoding_gaussian_matrix
        key, pk = (g.device, self.dtype), self._pk()         # the dense encoding and ``_coords``' constant, per device and dtype
        pe = pk.get(key)
        if pe is None:
            h, w = self.image_embedding_size
            y = (torch.arange(h, device=g.device, dtype=torch.float32) + 0.5) / h
            x = (torch.arange(w, device=g.device, dtype=torch.float32) + 0.5) / w
            grid = torch.stack([x[None, :].expand(h, w), y[:, None].expand(h, w)], dim=-1)
            pe = pk[key] = self.pe_layer.encode(grid).reshape(h * w, self.embed_dim).to(self.dtype).contiguous()
        return pe

    def _coords(self, pts: torch.Tensor) -> torch.Tensor:
        h, w = self.input_image_size
        key, pk = ("wh", pts.device), self._pk()  # uploaded once: a captured call (GroundedSam.predict_masks) cannot upload it
        wh = pk.get(key)
        if wh is None:
            wh = pk[key] = torch.tensor([w, h], dtype=torch.float32, device=pts.device)
        return self.pe_layer.encode((pts.float() + 0.5) / wh)

    @torch.no_grad()
    def forward(self, points: Optional[Tuple[torch.Tensor, torch.Tensor]], boxes: Optional[torch.Tensor], masks: Optional[torch.Tensor] = None):
        """-> (sparse [B, N, embed_dim], dense [embed_dim]: ``no_mask_embed``, the same for every pixel), in the storage dtype."""
        if masks is not None:
            raise L.OmgHipError("SamPromptEncoder: a mask prompt is not built (mask_downscaling has no kernel path); pass mask_input=None")
        if points is None and boxes is None:
            raise L.OmgHipError("SamPromptEncoder: give points, boxes or both")
        for t in ([points[0], points[1]] if points is not None else []) + ([boxes] if boxes is not None else []):
            if not t.is_cuda:
                raise L.OmgHipError("SamPromptEncoder needs its prompts on the MI355X (cuda/hip device); there is no CPU fallback")
        parts = []
        if points is not None:
            pts, labels = points
            if boxes is None:                                          # pad with a "not a point"
                pts = torch.cat([pts.float(), torch.zeros((pts.shape[0], 1, 2), dtype=torch.float32, device=pts.device)], dim=1)
                labels = torch.cat([labels, torch.full((labels.shape[0], 1), -1, dtype=labels.dtype, device=labels.device)], dim=1)
            e = self._coords(pts)
            lab = labels[..., None]
            e = torch.where(lab == -1, self.not_a_point_embed.weight.float().expand_as(e), e)
            e = e + (lab == 0) * self.point_embeddings[0].weight.float() + (lab == 1) * self.point_embeddings[1].weight.float()
            parts.append(e)
        if boxes is not None:
            e = self._coords(boxes.reshape(-1, 2, 2))
            e = e + torch.stack([self.point_embeddings[2].weight[0], self.point_embeddings[3].weight[0]]).float()
            parts.append(e)
        sparse = torch.cat(parts, dim=1).to(self.dtype)
        return sparse, self.no_mask_embed.weight.data[0]


# ---------------------------------------------------------------------------------------------- mask decoder
class _Attention(nn.Module):
    def __init__(self, dim, heads, downsample, dtype, device):
        super().__init__()
        self.internal_dim, self.num_heads = dim // downsample, heads
        d = self.internal_dim // heads
        if d not in (16, 32):
            raise L.OmgHipError(f"SamMaskDecoder: head_dim {d} has no kernel (omg_attn_small is built for 16 and 32)")
        self.q_proj = _Weight((self.internal_dim, dim), self.internal_dim, dtype, device)
        self.k_proj = _Weight((self.internal_dim, dim), self.internal_dim, dtype, device)
        self.v_proj = _Weight((self.internal_dim, dim), self.internal_dim, dtype, device)
        self.out_proj = _Weight((dim, self.internal_dim), dim, dtype, device)


class _MLPBlock(nn.Module):
    def __init__(self, dim, mlp_dim, dtype, device):
        super().__init__()
        self.lin1 = _Weight((mlp_dim, dim), mlp_dim, dtype, device)
        self.lin2 = _Weight((dim, mlp_dim), dim, dtype, device)


class _TwoWayBlock(nn.Module):
    def __init__(self, dim, heads, mlp_dim, dtype, device):
        super().__init__()
        self.self_attn = _Attention(dim, heads, 1, dtype, device)
        self.norm1 = _Weight((dim,), dim, dtype, device)
        self.cross_attn_token_to_image = _Attention(dim, heads, 2, dtype, device)
        self.norm2 = _Weight((dim,), dim, dtype, device)
        self.mlp = _MLPBlock(dim, mlp_dim, dtype, device)
        self.norm3 = _Weight((dim,), dim, dtype, device)
        self.norm4 = _Weight((dim,), dim, dtype, device)
        self.cross_attn_image_to_token = _Attention(dim, heads, 2, dtype, device)


class _TwoWayTransformer(nn.Module):
    def __init__(self, depth, dim, heads, mlp_dim, dtype, device):
        super().__init__()
        self.layers = nn.ModuleList([_TwoWayBlock(dim, heads, mlp_dim, dtype, device) for _ in range(depth)])
        self.final_attn_token_to_image = _Attention(dim, heads, 2, dtype, device)
        self.norm_final_attn = _Weight((dim,), dim, dtype, device)


class _MLP(nn.Module):
    def __init__(self, din, hidden, dout, n, dtype, device):
        super().__init__()
        dims = [din] + [hidden] * (n - 1) + [dout]
        self.layers = nn.ModuleList([_Weight((b, a), b, dtype, device) for a, b in zip(dims[:-1], dims[1:])])


class SamMaskDecoder(PackedCache):
    LN_EPS = 1e-5            # nn.LayerNorm's default (set_norm_eps overrides it per instance); LayerNorm2d of output_upscaling uses 1e-6

    def __init__(self, transformer_dim: int = 256, num_multimask_outputs: int = 3, depth: int = 2, num_heads: int = 8, mlp_dim: int = 2048,
                 iou_head_depth: int = 3, iou_head_hidden_dim: int = 256, dtype=torch.float16, device=None):
        super().__init__()
        D = transformer_dim
        if D % 64 or num_multimask_outputs + 1 > 4:
            raise L.OmgHipError("SamMaskDecoder: transformer_dim must be a multiple of 64 and at most 4 mask tokens (omg_sam_mask_logits)")
        self.transformer_dim, self.num_mask_tokens = D, num_multimask_outputs + 1
        self.transformer = _TwoWayTransformer(depth, D, num_heads, mlp_dim, dtype, device)
        self.iou_token = _Weight((1, D), 0, dtype, device)
        self.mask_tokens = _Weight((self.num_mask_tokens, D), 0, dtype, device)
        self.output_upscaling = _Seq({0: _Weight((D, D // 4, 2, 2), D // 4, dtype, device), 1: _Weight((D // 4,), D // 4, dtype, device),
                                      3: _Weight((D // 4, D // 8, 2, 2), D // 8, dtype, device)})
        self.output_hypernetworks_mlps = nn.ModuleList([_MLP(D, D, D // 8, 3, dtype, device) for _ in range(self.num_mask_tokens)])
        self.iou_prediction_head = _MLP(D, iou_head_hidden_dim, self.num_mask_tokens, iou_head_depth, dtype, device)

    def _pack(self) -> dict:
        """GEMM operands that are not the checkpoint's own tensors: transposed-convolution weights and the IoU head's last layer,
        padded from num_mask_tokens to omg_gemm's 8 output columns."""
        last = self.iou_prediction_head.layers[-1]
        w = torch.zeros((8, last.weight.shape[1]), dtype=last.weight.dtype, device=last.weight.device)
        b = torch.zeros((8,), dtype=last.weight.dtype, device=last.weight.device)
        w[:self.num_mask_tokens], b[:self.num_mask_tokens] = last.weight.data, last.bias.data
        return {"up0": ops.pack_convt2x2_weight(self.output_upscaling[0].weight.data),
                "up3": ops.pack_convt2x2_weight(self.output_upscaling[3].weight.data), "iou_w": w, "iou_b": b}

    # ------------------------------------------------------------------ pieces; x is [B, N, C], a GEMM is run per prompt
    @staticmethod
    def _lin(x, lin, residual=None, out=None, weight=None, bias=None):
        w = lin.weight.data if weight is None else weight
        b = lin.bias.data if bias is None else bias
        B, N, _ = x.shape
        if out is None:
            out = torch.empty((B, N, w.shape[0]), dtype=x.dtype, device=x.device)
        for i in range(B):
            ops.gemm(x[i], w, bias=b, residual=residual[i] if residual is not None else None, out=out[i])
        return out

    def _attn(self, a: _Attention, q, k, v, residual=None):
        """out_proj(attention(q_proj q, k_proj k, v_proj v)) (+ residual).  k and v are projected into the two halves of one buffer."""
        B, Nk, _ = k.shape
        I = a.internal_dim
        qp = self._lin(q, a.q_proj)
        kv = torch.empty((B, Nk, 2 * I), dtype=k.dtype, device=k.device)
        self._lin(k, a.k_proj, out=kv[:, :, :I])
        self._lin(v, a.v_proj, out=kv[:, :, I:])
        d = I // a.num_heads
        o = ops.attn_small(qp, kv[:, :, :I], kv[:, :, I:], a.num_heads, 1.0 / math.sqrt(d))
        return self._lin(o, a.out_proj, residual=residual)

    def _norm(self, x, n):
        return ops.layernorm(x, n.weight.data, n.bias.data, self.LN_EPS)

    def _mlp(self, x, mlp: _MLP, last_weight=None, last_bias=None):
        n = len(mlp.layers)
        for i, l in enumerate(mlp.layers):
            if i < n - 1:
                x = self._lin(x, l)
                ops.relu(x, out=x)
            else:
                x = self._lin(x, l, weight=last_weight, bias=last_bias)
        return x

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward_features(self, image_embeddings: torch.Tensor, image_pe: torch.Tensor, sparse_prompt_embeddings: torch.Tensor,
                         dense_prompt_embeddings: torch.Tensor, multimask_output: bool) -> Dict[str, torch.Tensor]:
        """image_embeddings: NHWC [1, H, W, D] (the encoder's "out"); image_pe [H * W, D]; sparse [B, N, D]; dense [D].
        -> {"layer{i}_queries" / "_keys", "final_queries", "upscaled" NHWC, "masks" fp32 [B, M, 4H, 4W], "iou" fp32 [B, M]}."""
        feat, sparse = image_embeddings, sparse_prompt_embeddings
        dt = self.iou_token.weight.dtype
        if not (feat.is_cuda and sparse.is_cuda):
            raise L.OmgHipError("SamMaskDecoder needs its inputs on the MI355X (cuda/hip device); there is no CPU fallback")
        D = self.transformer_dim
        if feat.dim() != 4 or feat.shape[0] != 1 or feat.shape[3] != D or feat.dtype != dt or sparse.dtype != dt or sparse.shape[2] != D:
            raise L.OmgHipError(f"SamMaskDecoder: image embedding must be NHWC [1, H, W, {D}] and prompts [B, N, {D}], both {dt}")
        _, H, W, _ = feat.shape
        B = sparse.shape[0]
        pk = self._pk()
        out: Dict[str, torch.Tensor] = {}
        tokens = torch.cat([torch.cat([self.iou_token.weight.data, self.mask_tokens.weight.data], dim=0)[None].expand(B, -1, -1), sparse], dim=1).contiguous()
        keys = (feat.reshape(H * W, D) + dense_prompt_embeddings)[None].expand(B, -1, -1).contiguous()
        key_pe = image_pe[None]
        queries = tokens
        t = self.transformer
        for i, l in enumerate(t.layers):
            if i == 0:
                queries = self._attn(l.self_attn, queries, queries, queries)
            else:
                q = queries + tokens
                queries = self._attn(l.self_attn, q, q, queries, residual=queries)
            queries = self._norm(queries, l.norm1)
            keys_pe = keys + key_pe                                    # the same operand for both cross-attentions of the layer
            queries = self._norm(self._attn(l.cross_attn_token_to_image, queries + tokens, keys_pe, keys, residual=queries), l.norm2)
            h = self._lin(queries, l.mlp.lin1)
            ops.relu(h, out=h)
            queries = self._norm(self._lin(h, l.mlp.lin2, residual=queries), l.norm3)
            keys = self._norm(self._attn(l.cross_attn_image_to_token, keys_pe, queries + tokens, queries, residual=keys), l.norm4)
            out[f"layer{i}_queries"], out[f"layer{i}_keys"] = queries, keys
        queries = self._norm(self._attn(t.final_attn_token_to_image, queries + tokens, keys + key_pe, keys, residual=queries), t.norm_final_attn)
        out["final_queries"] = queries

        up0, ln, up3 = self.output_upscaling[0], self.output_upscaling[1], self.output_upscaling[3]
        mid = torch.empty((B, 2 * H, 2 * W, D // 4), dtype=dt, device=feat.device)
        up = torch.empty((B, 4 * H, 4 * W, D // 8), dtype=dt, device=feat.device)
        for b in range(B):
            ops.convt2x2_ln_gelu(keys[b].view(1, H, W, D), pk["up0"], up0.bias.data, ln_weight=ln.weight.data, ln_bias=ln.bias.data, eps=1e-6,
                                 gelu=True, out=mid[b:b + 1])
            ops.convt2x2_ln_gelu(mid[b:b + 1], pk["up3"], up3.bias.data, gelu=True, out=up[b:b + 1])
        out["upscaled"] = up
        which = range(1, self.num_mask_tokens) if multimask_output else range(0, 1)
        hyper = torch.stack([self._mlp(queries[:, 1 + m:2 + m, :], self.output_hypernetworks_mlps[m])[:, 0] for m in which], dim=1).contiguous()
        out["hyper"] = hyper
        out["masks"] = ops.sam_mask_logits(hyper, up)
        iou = self._mlp(queries[:, 0:1, :], self.iou_prediction_head, last_weight=pk["iou_w"], last_bias=pk["iou_b"])[:, 0, :self.num_mask_tokens]
        out["iou"] = iou[:, which.start:which.stop].float()
        return out

    def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output: bool):
        """-> (low-resolution mask logits fp32 [B, M, 4H, 4W], IoU predictions fp32 [B, M]); M = 3 (masks 1..3) or 1 (mask 0)."""
        f = self.forward_features(image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output)
        return f["masks"], f["iou"]


# ---------------------------------------------------------------------------------------------- the model and the predictor
class EfficientViTSam(nn.Module):
    mask_threshold: float = 0.0
    image_format: str = "RGB"
    pixel_mean = (123.675, 116.28, 103.53)
    pixel_std = (58.395, 57.12, 57.375)

    def __init__(self, image_encoder: EfficientViTSamImageEncoder, prompt_encoder: SamPromptEncoder, mask_decoder: SamMaskDecoder,
                 image_size: Tuple[int, int] = (1024, 512)):
        super().__init__()
        self.image_encoder, self.prompt_encoder, self.mask_decoder = image_encoder, prompt_encoder, mask_decoder
        self.image_size = tuple(image_size)             # (the frame of prompts and input_size, the side of the encoder's input)

    @staticmethod
    def get_preprocess_shape(oldh: int, oldw: int, long_side_length: int) -> Tuple[int, int]:
        scale = long_side_length * 1.0 / max(oldh, oldw)
        return int(oldh * scale + 0.5), int(oldw * scale + 0.5)

    def _device_lut(self, dtype, device) -> torch.Tensor:
        key = (dtype, torch.device(device))
        if getattr(self, "_lut_key", None) != key:
            from . import image_prep
            self._lut_key = key
            self._lut_t = image_prep.lut_unit_mean_std([v / 255 for v in self.pixel_mean], [v / 255 for v in self.pixel_std], dtype, device)
        return self._lut_t

    def preprocess_device(self, image: torch.Tensor, dtype: torch.dtype = torch.float32, want_image: bool = True):
        """:meth:`preprocess` of a cuda uint8 [H, W, 3] image on the device (ops.image_prep: Pillow's bilinear resize bit for bit, the
        normalisation as a lookup table of the host expression, pad and cast in the same launch) -> (the resized uint8 image or None,
        the encoder's input [1, 3, S, S] in ``dtype``)."""
        from . import image_prep
        if not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
            raise L.OmgHipError(f"EfficientViTSam.preprocess: a tensor image is a cuda uint8 [H, W, 3] tensor, got {image.dtype} "
                                f"{tuple(image.shape)} on {image.device}")
        image = image.contiguous()
        side = self.image_size[1]
        h, w = int(image.shape[0]), int(image.shape[1])
        th, tw = (h, w) if max(h, w) == side else self.get_preprocess_shape(h, w, side)
        x = ops.image_prep(image, (th, tw), image_prep.BILINEAR, lut=self._device_lut(dtype, image.device), pad_hw=(side, side))[None]
        resized = None
        if want_image:
            resized = image if (th, tw) == (h, w) else ops.image_prep(image, (th, tw), image_prep.BILINEAR)
        return resized, x

    def preprocess(self, image):
        """HWC uint8 RGB -> (the resized uint8 image, the encoder's input [1, 3, S, S] fp32 on the host): the long side resized to
        ``image_size[1]`` through PIL (bilinear, as torchvision resizes a PIL image), x / 255, mean / std, zero pad at the right and bottom.
        A cuda uint8 tensor gives the same two, on the device (:meth:`preprocess_device`)."""
        if isinstance(image, torch.Tensor):
            return self.preprocess_device(image)
        from PIL import Image
        side = self.image_size[1]
        h, w, _ = image.shape
        if max(h, w) != side:
            th, tw = self.get_preprocess_shape(h, w, side)
            image = np.array(Image.fromarray(np.ascontiguousarray(image)).resize((tw, th), Image.BILINEAR))
        x = torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1).float().div(255)
        mean = torch.tensor([v / 255 for v in self.pixel_mean], dtype=torch.float32)[:, None, None]      # divided in double, as the reference's lists
        std = torch.tensor([v / 255 for v in self.pixel_std], dtype=torch.float32)[:, None, None]
        x = (x - mean) / std
        x = torch.nn.functional.pad(x, (0, side - x.shape[2], 0, side - x.shape[1]), value=0.0)
        return image, x[None]

    def postprocess_masks(self, masks: torch.Tensor, input_size, original_size, threshold: Optional[float] = None) -> torch.Tensor:
        """fp32 low-resolution logits [B, M, h, w] -> fp32 logits at ``original_size`` (or uint8 0 / 1 against ``threshold``)."""
        return ops.sam_postprocess(masks.contiguous(), self.image_size[0], input_size, original_size, threshold=threshold)


def efficientvit_sam(name: str, dtype=torch.float16, device=None) -> EfficientViTSam:
    """The reference's efficientvit_sam_l0 / l1 / l2 (512 x 512 encoder input, prompts in a 1024 frame); weights are left to load_state_dict."""
    cfg = EfficientViTSamConfig.variant(name)           # refuses the xl names
    return EfficientViTSam(EfficientViTSamImageEncoder(cfg, dtype=dtype, device=device),
                           SamPromptEncoder(256, (64, 64), (1024, 1024), 16, dtype=dtype, device=device),
                           SamMaskDecoder(256, 3, 2, 8, 2048, 3, 256, dtype=dtype, device=device), image_size=(1024, 512))


def _build(cfg: EfficientViTSamConfig, image_size: int, dtype, device) -> EfficientViTSam:
    """build_efficientvit_sam of the reference (sam.py:520-544): the same prompt encoder and mask decoder behind every image encoder."""
    return EfficientViTSam(EfficientViTSamImageEncoder(cfg, dtype=dtype, device=device),
                           SamPromptEncoder(256, (64, 64), (1024, 1024), 16, dtype=dtype, device=device),
                           SamMaskDecoder(256, 3, 2, 8, 2048, 3, 256, dtype=dtype, device=device), image_size=(1024, image_size))


def efficientvit_sam_xl0(image_size: int = 1024, dtype=torch.float16, device=None) -> EfficientViTSam:
    """The reference's efficientvit_sam_xl0 (sam.py:604-627): six stages, att@3 blocks, a 1024 x 1024 encoder input."""
    return _build(EfficientViTSamConfig.xl0(), image_size, dtype, device)


def efficientvit_sam_xl1(image_size: int = 1024, dtype=torch.float16, device=None) -> EfficientViTSam:
    """The reference's efficientvit_sam_xl1 (sam.py:630-653), the segmenter every script of the reference builds."""
    return _build(EfficientViTSamConfig.xl1(), image_size, dtype, device)


def set_norm_eps(model: nn.Module, eps: float) -> None:
    """set_norm_eps of the reference (models/nn/norm.py:153-157) on this package's holders: every BatchNorm, the encoder's LayerNorm2d,
    LiteMLA's proj.norm and the two-way transformer's LayerNorms get ``eps``.  output_upscaling's LayerNorm2d keeps its 1e-6: it is
    segment_anything's class, no nn.LayerNorm, and the reference's call leaves it alone.  BatchNorm is folded when the packed weights
    are built, so every packed-weight cache is dropped."""
    for m in model.modules():
        if isinstance(m, (_ev._BatchNorm, _ev._LayerNorm)):
            m.eps = eps
        elif isinstance(m, LiteMLA) and m.proj.norm is not None:
            m.proj.norm.eps = eps
        elif isinstance(m, SamMaskDecoder):
            m.LN_EPS = eps
        if isinstance(m, PackedCache):
            m.invalidate_packed()


def create_sam_model(name: str, pretrained: bool = True, weight_url: Optional[str] = None, dtype=torch.float16, device=None) -> EfficientViTSam:
    """create_sam_model of the reference (sam_model_zoo.py:26-53): ``name`` up to its first "-" is l0 | l1 | l2 | xl0 | xl1; the model is
    built, every norm's eps is set to 1e-6, and with ``pretrained`` the checkpoint at ``weight_url`` is loaded (there is no model zoo
    directory to fall back on)."""
    builders = {"l0": lambda: efficientvit_sam("l0", dtype=dtype, device=device), "l1": lambda: efficientvit_sam("l1", dtype=dtype, device=device),
                "l2": lambda: efficientvit_sam("l2", dtype=dtype, device=device),
                "xl0": lambda: efficientvit_sam_xl0(dtype=dtype, device=device), "xl1": lambda: efficientvit_sam_xl1(dtype=dtype, device=device)}
    model_id = name.split("-")[0]
    if model_id not in builders:
        raise ValueError(f"Do not find {name} in the model zoo. List of models: {list(builders)}")
    if pretrained and weight_url is None:
        raise ValueError(f"Do not find the pretrained weight of {name}: pass weight_url")
    model = builders[model_id]()
    set_norm_eps(model, 1e-6)
    if pretrained:
        weight = torch.load(weight_url, map_location="cpu")
        if "state_dict" in weight:
            weight = weight["state_dict"]
        model.load_state_dict(weight)
    return model


class EfficientViTSamPredictor:
    def __init__(self, sam_model: EfficientViTSam) -> None:
        self.model = sam_model
        self.reset_image()

    @property
    def transform(self):
        return self

    @property
    def device(self):
        return self.model.mask_decoder.iou_token.weight.device

    def reset_image(self) -> None:
        self.is_image_set = False
        self.features = None
        self.original_size = None
        self.input_size = None

    def apply_coords(self, coords: np.ndarray, im_size=None) -> np.ndarray:
        old_h, old_w = self.original_size
        new_h, new_w = self.input_size
        coords = np.array(coords, dtype=float, copy=True)
        coords[..., 0] = coords[..., 0] * (new_w / old_w)
        coords[..., 1] = coords[..., 1] * (new_h / old_h)
        return coords

    def apply_boxes(self, boxes: np.ndarray, im_size=None) -> np.ndarray:
        return self.apply_coords(np.asarray(boxes).reshape(-1, 2, 2)).reshape(-1, 4)

    def apply_coords_torch(self, coords: torch.Tensor, im_size=None) -> torch.Tensor:
        """apply_coords on a tensor (segment_anything's ResizeLongestSide has it, and the reference's YOLO-World path calls it)."""
        old_h, old_w = self.original_size
        new_h, new_w = self.input_size
        coords = coords.clone().to(torch.float)
        coords[..., 0] = coords[..., 0] * (new_w / old_w)
        coords[..., 1] = coords[..., 1] * (new_h / old_h)
        return coords

    def apply_boxes_torch(self, boxes: torch.Tensor, im_size=None) -> torch.Tensor:
        return self.apply_coords_torch(boxes.reshape(-1, 2, 2)).reshape(-1, 4)

    def _set_sizes(self, hw) -> None:
        """``original_size`` and ``input_size`` (the image's size in the prompts' frame) of an H x W image."""
        self.original_size = (int(hw[0]), int(hw[1]))
        self.input_size = self.model.get_preprocess_shape(*self.original_size, long_side_length=self.model.image_size[0])

    def set_image(self, image, image_format: str = "RGB") -> None:
        """``image``: HWC uint8, a numpy array (the host preprocessing) or a cuda tensor (the same bits from ops.image_prep's launches)."""
        assert image_format in ["RGB", "BGR"], f"image_format must be in ['RGB', 'BGR'], is {image_format}."
        if not self.device.type == "cuda":
            raise L.OmgHipError("EfficientViTSamPredictor needs its model on the MI355X (cuda/hip device); there is no CPU fallback")
        dt = self.model.mask_decoder.iou_token.weight.dtype
        if isinstance(image, torch.Tensor):
            if image_format != self.model.image_format:
                image = image.flip(-1)
            _, x = self.model.preprocess_device(image, dtype=dt, want_image=False)
            self.reset_image()
            self._set_sizes(image.shape[:2])
            self.features = self.model.image_encoder.forward_features(x)["out"]        # NHWC
            self.is_image_set = True
            return
        if image_format != self.model.image_format:
            image = image[..., ::-1]
        self.reset_image()
        self._set_sizes(image.shape[:2])
        _, x = self.model.preprocess(image)
        self.features = self.model.image_encoder.forward_features(x.to(self.device, dt))["out"]        # NHWC
        self.is_image_set = True

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output: bool = True, return_logits: bool = False):
        """Prompts in the original image's pixels -> (masks [C, H, W] bool or fp32 logits, IoU predictions [C], low-resolution logits
        [C, 256, 256]) as numpy arrays."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        if mask_input is not None:
            raise L.OmgHipError("EfficientViTSamPredictor: a mask prompt is not built; pass mask_input=None")
        device = self.device
        coords_torch = labels_torch = box_torch = None
        if point_coords is not None:
            assert point_labels is not None, "point_labels must be supplied if point_coords is supplied."
            coords_torch = torch.as_tensor(self.apply_coords(point_coords), dtype=torch.float, device=device)[None, :, :]
            labels_torch = torch.as_tensor(point_labels, dtype=torch.int, device=device)[None, :]
        if box is not None:
            box_torch = torch.as_tensor(self.apply_boxes(box), dtype=torch.float, device=device)[None, :]
        masks, iou, low = self.predict_torch(coords_torch, labels_torch, box_torch, None, multimask_output, return_logits=return_logits)
        return masks[0].cpu().numpy(), iou[0].cpu().numpy(), low[0].cpu().numpy()

    @torch.no_grad()
    def predict_torch(self, point_coords=None, point_labels=None, boxes=None, mask_input=None, multimask_output: bool = True,
                      return_logits: bool = False):
        """Batched prompts already in the input frame (apply_coords / apply_boxes) -> (masks [B, C, H, W] bool or fp32 logits,
        IoU predictions [B, C], low-resolution logits [B, C, 256, 256]) on the device."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        if mask_input is not None:
            raise L.OmgHipError("EfficientViTSamPredictor: a mask prompt is not built; pass mask_input=None")
        m = self.model
        points = (point_coords, point_labels) if point_coords is not None else None
        if boxes is not None and boxes.dim() == 3:
            boxes = boxes.reshape(boxes.shape[0], -1)
        sparse, dense = m.prompt_encoder(points=points, boxes=boxes, masks=None)
        low, iou = m.mask_decoder(self.features, m.prompt_encoder.get_dense_pe(), sparse, dense, multimask_output)
        if return_logits:
            masks = m.postprocess_masks(low, self.input_size, self.original_size)
        else:
            masks = m.postprocess_masks(low, self.input_size, self.original_size, threshold=m.mask_threshold).bool()
        return masks, iou, low
