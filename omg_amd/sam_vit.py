"""SAM's ViT image encoder (vit_b / vit_l / vit_h) on the HIP kernels: ``segment_anything.modeling.ImageEncoderViT``.

The module tree and parameter names are those of a ``sam_vit_*.pth`` checkpoint (``patch_embed.proj``, ``pos_embed``,
``blocks.{i}.norm1 / attn.qkv / attn.proj / attn.rel_pos_h / attn.rel_pos_w / norm2 / mlp.lin1 / mlp.lin2``, ``neck.0 .. 3``), so its
``image_encoder.*`` part loads key for key.  NCHW 16-bit in (already resized, normalised and padded), NCHW ``[B, 256, 64, 64]`` out;
image-order NHWC rows ``[B * 64 * 64, D]`` inside.

  patch embedding (16 x 16, stride 16)   -> view ops + omg_gemm on the [4096, 768] patches: bias, and pos_embed as the residual
  LayerNorm (eps 1e-6), LayerNorm2d      -> omg_layernorm on the rows
  qkv / proj / lin1 / lin2, neck.0       -> omg_gemm: bias and the block's shortcut in its epilogue
  attention                              -> omg_attn_relpos on the fused QKV rows: the decomposed relative-position bias inside the
                                            kernel, 14 x 14 windows indexed in place — no window_partition / unpartition pass, no
                                            padded 70 x 70 buffer (a padded position is a key with k | v = the k | v slices of the QKV
                                            bias, which is what zero padding AFTER norm1 makes of it), and no [heads, 4096, 4096] bias
                                            or score tensor for the global layers
  GELU of the MLP                        -> omg_gelu_erf, in place
  neck.2 (3 x 3, no bias)                -> omg_conv3x3_nhwc_act

A relative-position table must have the layer's own length (2 S - 1): the reference interpolates it otherwise, which only happens at
input sizes other than the model's.  Inference only.  There is no CPU path: ``forward`` on a CPU tensor raises.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._checkpoint import PackedCache, Seq as _Seq, Weight as _Weight, param as _param

__all__ = ["SamImageEncoderViT"]


class _PatchEmbed(nn.Module):
    def __init__(self, patch, cin, dim, dtype, device):
        super().__init__()
        self.proj = _Weight((dim, cin, patch, patch), dim, dtype, device)


class _Attention(nn.Module):
    def __init__(self, dim, heads, size: Tuple[int, int], dtype, device):
        super().__init__()
        self.num_heads, self.input_size = heads, size
        d = dim // heads
        if dim % heads or d not in (64, 80):
            raise L.OmgHipError(f"SamImageEncoderViT: head_dim {dim / heads:g} has no kernel (omg_attn_relpos is built for 64 and 80)")
        self.qkv = _Weight((3 * dim, dim), 3 * dim, dtype, device)
        self.proj = _Weight((dim, dim), dim, dtype, device)
        self.rel_pos_h = _param((2 * size[0] - 1, d), dtype, device)
        self.rel_pos_w = _param((2 * size[1] - 1, d), dtype, device)


class _MLP(nn.Module):
    def __init__(self, dim, mlp_dim, dtype, device):
        super().__init__()
        self.lin1 = _Weight((mlp_dim, dim), mlp_dim, dtype, device)
        self.lin2 = _Weight((dim, mlp_dim), dim, dtype, device)


class _Block(nn.Module):
    def __init__(self, dim, heads, mlp_ratio, window, grid, dtype, device):
        super().__init__()
        self.window_size = window                         # 0: global attention
        self.norm1 = _Weight((dim,), dim, dtype, device)
        self.attn = _Attention(dim, heads, (window, window) if window else (grid, grid), dtype, device)
        self.norm2 = _Weight((dim,), dim, dtype, device)
        self.mlp = _MLP(dim, int(dim * mlp_ratio), dtype, device)


class SamImageEncoderViT(PackedCache):
    LN_EPS = 1e-6

    def __init__(self, img_size: int = 1024, patch_size: int = 16, in_chans: int = 3, embed_dim: int = 768, depth: int = 12, num_heads: int = 12,
                 mlp_ratio: float = 4.0, out_chans: int = 256, window_size: int = 14, global_attn_indexes: Sequence[int] = (2, 5, 8, 11),
                 dtype=torch.float16, device=None):
        super().__init__()
        if img_size % patch_size or (in_chans * patch_size * patch_size) % 8 or embed_dim % 8 or out_chans % 8:
            raise L.OmgHipError("SamImageEncoderViT: img_size must be a multiple of patch_size; patch, embed_dim and out_chans multiples of 8 (omg_gemm)")
        if window_size < 0 or window_size * window_size > 256:
            raise L.OmgHipError(f"SamImageEncoderViT: window_size {window_size} has no kernel (omg_attn_relpos takes windows of at most 256 positions)")
        self.img_size, self.patch_size, self.in_chans, self.embed_dim, self.out_chans = img_size, patch_size, in_chans, embed_dim, out_chans
        self.grid = img_size // patch_size
        self.global_attn_indexes = tuple(global_attn_indexes)
        self.patch_embed = _PatchEmbed(patch_size, in_chans, embed_dim, dtype, device)
        self.pos_embed = _param((1, self.grid, self.grid, embed_dim), dtype, device)
        self.blocks = nn.ModuleList([_Block(embed_dim, num_heads, mlp_ratio, 0 if i in self.global_attn_indexes else window_size, self.grid, dtype, device)
                                     for i in range(depth)])
        self.neck = _Seq([_Weight((out_chans, embed_dim, 1, 1), 0, dtype, device), _Weight((out_chans,), out_chans, dtype, device),
                          _Weight((out_chans, out_chans, 3, 3), 0, dtype, device), _Weight((out_chans,), out_chans, dtype, device)])

    # ------------------------------------------------------------------ kernel operands that are not the checkpoint's own tensors, built once
    def _pack(self) -> dict:
        D = self.embed_dim
        return {"patch": self.patch_embed.proj.weight.data.reshape(D, -1).contiguous(),
                "neck0": self.neck[0].weight.data.reshape(self.out_chans, D).contiguous(),
                "neck2": self.neck[2].weight.data.permute(0, 2, 3, 1).contiguous()}

    @property
    def dtype(self):
        return self.pos_embed.dtype

    def _check_tables(self) -> None:
        for i, blk in enumerate(self.blocks):
            S = blk.window_size or self.grid
            for name in ("rel_pos_h", "rel_pos_w"):
                n = getattr(blk.attn, name).shape[0]
                if n != 2 * S - 1:
                    raise L.OmgHipError(f"SamImageEncoderViT: blocks.{i}.attn.{name} has {n} rows, the layer needs {2 * S - 1} "
                                        "(interpolating a relative-position table is not built)")

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward_features(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """NCHW input -> {"patch_embed", "block0" .. "block{depth-1}", "neck0", "neck1", "neck2", "out"}: NHWC tensors ("out" is the
        embedding [B, grid, grid, out_chans] before the final permute)."""
        self._check_tables()
        if not x.is_cuda:
            raise L.OmgHipError("SamImageEncoderViT needs its input on the MI355X (cuda/hip device); there is no CPU fallback")
        dt, G, P, D = self.dtype, self.grid, self.patch_size, self.embed_dim
        if x.dtype != dt or x.dim() != 4 or tuple(x.shape[1:]) != (self.in_chans, self.img_size, self.img_size):
            raise L.OmgHipError(f"SamImageEncoderViT: input must be [B, {self.in_chans}, {self.img_size}, {self.img_size}] in {dt}")
        B = x.shape[0]
        pk = self._pk()
        feats: Dict[str, torch.Tensor] = {}
        patches = x.view(B, self.in_chans, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, -1)
        h = torch.empty((B * G * G, D), dtype=dt, device=x.device)
        pos = self.pos_embed.data.view(G * G, D)
        for b in range(B):
            r = slice(b * G * G, (b + 1) * G * G)
            ops.gemm(patches[r], pk["patch"], bias=self.patch_embed.proj.bias.data, residual=pos, out=h[r])
        feats["patch_embed"] = h.view(B, G, G, D)
        for i, blk in enumerate(self.blocks):
            a = blk.attn
            d = D // a.num_heads
            y = ops.layernorm(h, blk.norm1.weight.data, blk.norm1.bias.data, self.LN_EPS)
            qkv = ops.gemm(y, a.qkv.weight.data, bias=a.qkv.bias.data)
            o = ops.attn_relpos(qkv, B, G, G, a.num_heads, a.rel_pos_h.data, a.rel_pos_w.data, 1.0 / math.sqrt(d), window=blk.window_size,
                                pad_kv=a.qkv.bias.data[D:] if blk.window_size else None)
            h = ops.gemm(o, a.proj.weight.data, bias=a.proj.bias.data, residual=h)
            y = ops.layernorm(h, blk.norm2.weight.data, blk.norm2.bias.data, self.LN_EPS)
            t = ops.gemm(y, blk.mlp.lin1.weight.data, bias=blk.mlp.lin1.bias.data)
            ops.gelu_erf(t, out=t)
            h = ops.gemm(t, blk.mlp.lin2.weight.data, bias=blk.mlp.lin2.bias.data, residual=h)
            feats[f"block{i}"] = h.view(B, G, G, D)
        n = self.neck
        t = ops.gemm(h, pk["neck0"])
        feats["neck0"] = t.view(B, G, G, self.out_chans)
        t = ops.layernorm(t, n[1].weight.data, n[1].bias.data, self.LN_EPS)
        feats["neck1"] = t.view(B, G, G, self.out_chans)
        t = ops.conv3x3_nhwc_act(t.view(B, G, G, self.out_chans), pk["neck2"])
        feats["neck2"] = t
        feats["out"] = ops.layernorm(t, n[3].weight.data, n[3].bias.data, self.LN_EPS)
        return feats

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (B, 3, S, S), 16-bit, resized / normalised / padded -> the image embedding (B, out_chans, grid, grid) (a permuted view of the NHWC result)."""
        return self.forward_features(x)["out"].permute(0, 3, 1, 2)
