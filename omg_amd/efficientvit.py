"""EfficientViT-SAM's image encoder on the HIP kernels: the segmenter's cost between the two stages.

Mirrors ``EfficientViTSamImageEncoder`` of the reference (src/efficientvit/models/efficientvit/sam.py: an ``EfficientViTLargeBackbone``,
a ``SamNeck`` and a ``LayerNorm2d``) — the same module tree, hence the same state-dict keys (``backbone.stages.{s}.op_list.{i}...``,
``neck.input_ops / middle / output_ops``, ``norm``), so the ``image_encoder.*`` part of an ``efficientvit_sam_l0 / l1 / l2``
checkpoint loads key for key.  NCHW 16-bit in (already resized, normalised and padded: SamResize, the mean / std and SamPad stay
with the caller), NCHW ``[B, 256, 64, 64]`` out; NHWC rows inside, as LiteMLA.

  3x3 convolutions (stem, ResBlock, FusedMBConv.spatial_conv)  -> omg_conv3x3_nhwc_act: bias, GELU, residual in its epilogue
  1x1 convolutions                                              -> omg_gemm: bias and the ResidualBlock shortcut in its epilogue
  MBConv.depth_conv                                             -> omg_dwconv3x3_act, which also applies the GELU of the 1x1
                                                                   inverted_conv in front of it while it loads (the reference's "gelu"
                                                                   is the tanh form, models/nn/act.py; omg_gemm's GELU epilogue is the
                                                                   erf form of GEGLU, so the activation cannot ride on that GEMM)
  EfficientViTBlock.context_module                              -> omg_amd.litemla.LiteMLA ("att": scales (5,); "att@3": scales (3,));
                                                                   the xl recipes run its aggregation as omg_litemla_aggreg
  SamNeck fusion  sum_i upsample(conv1x1(stage_i))              -> omg_gemm + omg_upsample_add_nhwc (bicubic, as UpSampleLayer's default)
  LayerNorm2d                                                   -> omg_layernorm on the NHWC rows

BatchNorm (eval mode) is folded into the preceding convolution when the packed weights are built: in fp32, rounded once.
Inference only.  There is no CPU path: ``forward`` on a CPU tensor raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._checkpoint import PackedCache
from .litemla import LiteMLA


@dataclass(frozen=True)
class EfficientViTSamConfig:
    """An EfficientViTLargeBackbone (stage s: one stride-2 block, then depth_list[s] blocks of block_list[s]) and a SamNeck over the
    stages ``neck_fids``.  The defaults are the l-series'; ``xl0()`` / ``xl1()`` are the six-stage recipes of the reference's
    efficientvit_sam_xl0 / _xl1 (models/efficientvit/sam.py:604-653)."""
    width_list: Tuple[int, ...]
    depth_list: Tuple[int, ...]
    block_list: Tuple[str, ...] = ("res", "fmb", "fmb", "mb", "att")
    expand_list: Tuple[float, ...] = (1, 4, 4, 4, 6)
    fewer_norm_list: Tuple[bool, ...] = (False, False, False, True, True)
    qkv_dim: int = 32
    neck_fids: Tuple[int, ...] = (4, 3, 2)        # summed in this order
    head_width: int = 256
    head_depth: int = 4
    neck_expand: float = 1
    neck_middle: str = "fmb"
    out_dim: int = 256
    grid: int = 64                                # the neck resizes every input to grid x grid
    fused_aggreg: bool = False                    # LiteMLA's aggregation as omg_litemla_aggreg (no block-diagonal weight image)

    @staticmethod
    def variant(name: str) -> "EfficientViTSamConfig":
        name = name.lower()
        if name.startswith("xl"):
            raise L.OmgHipError(f"EfficientViT-SAM {name}: the xl variants (six stages, att@3 blocks, 1024^2 input) are not built by name "
                                "here; use efficientvit_sam_xl0 / efficientvit_sam_xl1 / create_sam_model, or EfficientViTSamConfig.xl0() / .xl1()")
        depth = {"l0": ((1, 1, 1, 4, 4), 4), "l1": ((1, 1, 1, 6, 6), 8), "l2": ((1, 2, 2, 8, 8), 12)}
        if name not in depth:
            raise L.OmgHipError(f"unknown EfficientViT-SAM variant {name!r}; use l0, l1 or l2")
        d, hd = depth[name]
        return EfficientViTSamConfig(width_list=(32, 64, 128, 256, 512), depth_list=d, head_depth=hd)

    @staticmethod
    def _xl(depth_list, head_depth) -> "EfficientViTSamConfig":
        return EfficientViTSamConfig(width_list=(32, 64, 128, 256, 512, 1024), depth_list=depth_list,
                                     block_list=("res", "fmb", "fmb", "fmb", "att@3", "att@3"), expand_list=(1, 4, 4, 4, 4, 6),
                                     fewer_norm_list=(False, False, False, False, True, True), neck_fids=(5, 4, 3), head_depth=head_depth,
                                     neck_expand=4, fused_aggreg=True)

    @staticmethod
    def xl0() -> "EfficientViTSamConfig":
        return EfficientViTSamConfig._xl((0, 1, 1, 2, 3, 3), 6)

    @staticmethod
    def xl1() -> "EfficientViTSamConfig":
        return EfficientViTSamConfig._xl((1, 2, 2, 4, 6, 6), 12)


# ---------------------------------------------------------------------------------------------- the reference's module tree, as holders of weights
class _Conv(nn.Module):
    def __init__(self, shape, bias, dtype, device):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(shape, dtype=dtype, device=device), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(shape[0], dtype=dtype, device=device), requires_grad=False) if bias else None


class _BatchNorm(nn.Module):
    def __init__(self, c, dtype, device):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c, dtype=dtype, device=device), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(c, dtype=dtype, device=device), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(c, dtype=torch.float32, device=device))
        self.register_buffer("running_var", torch.ones(c, dtype=torch.float32, device=device))
        self.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.long, device=device))
        self.eps = 1e-5


class ConvLayer(nn.Module):
    """ConvLayer (models/nn/ops.py:37-78): ``conv`` (+ ``norm`` = BatchNorm2d) (+ GELU).  kind: "c3" dense 3x3, "dw" depthwise 3x3, "pw" 1x1."""

    def __init__(self, cin, cout, kind, stride, bias, norm, act, dtype, device):
        super().__init__()
        self.kind, self.stride, self.act, self.cin, self.cout = kind, stride, act, cin, cout
        shape = {"c3": (cout, cin, 3, 3), "dw": (cout, 1, 3, 3), "pw": (cout, cin, 1, 1)}[kind]
        self.conv = _Conv(shape, bias, dtype, device)
        self.norm = _BatchNorm(cout, dtype, device) if norm else None

    def folded(self):
        """(weight [Cout, Cin | 1, k, k] fp32, bias [Cout] fp32 or None): the BatchNorm of eval mode folded in, not yet rounded."""
        w = self.conv.weight.data.float()
        b = self.conv.bias.data.float() if self.conv.bias is not None else None
        if self.norm is not None:
            n = self.norm
            a = n.weight.data.float() / torch.sqrt(n.running_var.float() + n.eps)
            w = w * a[:, None, None, None]
            b = n.bias.data.float() + ((b if b is not None else 0.0) - n.running_mean.float()) * a
        return w, b

    def packed(self):
        """The kernel's operand layout in the storage dtype: c3 [Cout, 3, 3, Cin]; dw [9, C] tap-major; pw [Cout, Cin]."""
        w, b = self.folded()
        dt = self.conv.weight.dtype
        if self.kind == "c3":
            w = w.permute(0, 2, 3, 1)
        elif self.kind == "dw":
            w = w.reshape(self.cout, 9).t()
        else:
            w = w.reshape(self.cout, self.cin)
        return w.to(dt).contiguous(), (b.to(dt).contiguous() if b is not None else None)


class ResBlock(nn.Module):
    def __init__(self, cin, cout, stride, fewer_norm, dtype, device):
        super().__init__()
        b, n = ((True, False), (False, True)) if fewer_norm else ((False, False), (True, True))
        self.conv1 = ConvLayer(cin, cin, "c3", stride, b[0], n[0], True, dtype, device)
        self.conv2 = ConvLayer(cin, cout, "c3", 1, b[1], n[1], False, dtype, device)


class FusedMBConv(nn.Module):
    def __init__(self, cin, cout, stride, expand, fewer_norm, dtype, device):
        super().__init__()
        b, n = ((True, False), (False, True)) if fewer_norm else ((False, False), (True, True))
        mid = round(cin * expand)
        self.spatial_conv = ConvLayer(cin, mid, "c3", stride, b[0], n[0], True, dtype, device)
        self.point_conv = ConvLayer(mid, cout, "pw", 1, b[1], n[1], False, dtype, device)


class MBConv(nn.Module):
    def __init__(self, cin, cout, stride, expand, fewer_norm, dtype, device):
        super().__init__()
        b, n = ((True, True, False), (False, False, True)) if fewer_norm else ((False,) * 3, (True,) * 3)
        mid = round(cin * expand)
        self.inverted_conv = ConvLayer(cin, mid, "pw", 1, b[0], n[0], True, dtype, device)
        self.depth_conv = ConvLayer(mid, mid, "dw", stride, b[1], n[1], True, dtype, device)
        self.point_conv = ConvLayer(mid, cout, "pw", 1, b[2], n[2], False, dtype, device)


class ResidualBlock(nn.Module):
    """ResidualBlock(main, IdentityLayer() | None): ``shortcut`` holds no weights, so it is a flag here."""

    def __init__(self, main, shortcut: bool):
        super().__init__()
        self.main = main
        self.has_shortcut = shortcut


class EfficientViTBlock(nn.Module):
    def __init__(self, c, dim, expand, dtype, device, scales=(5,), aggreg="gemm"):
        super().__init__()
        self.context_module = ResidualBlock(LiteMLA(c, c, dim=dim, norm=(None, "bn2d"), scales=scales, dtype=dtype, device=device, aggreg=aggreg), True)
        self.local_module = ResidualBlock(MBConv(c, c, 1, expand, True, dtype, device), True)


class OpSequential(nn.Module):
    def __init__(self, ops_):
        super().__init__()
        self.op_list = nn.ModuleList(ops_)


def _local_block(block, cin, cout, stride, expand, fewer_norm, dtype, device):
    if block == "res":
        return ResBlock(cin, cout, stride, fewer_norm, dtype, device)
    if block == "fmb":
        return FusedMBConv(cin, cout, stride, expand, fewer_norm, dtype, device)
    if block == "mb":
        return MBConv(cin, cout, stride, expand, fewer_norm, dtype, device)
    raise L.OmgHipError(f"EfficientViT: unknown block type {block!r}")


class _Backbone(nn.Module):
    def __init__(self, cfg: EfficientViTSamConfig, dtype, device):
        super().__init__()
        w, d = cfg.width_list, cfg.depth_list
        stage0 = [ConvLayer(3, w[0], "c3", 2, False, True, True, dtype, device)]
        for _ in range(d[0]):
            stage0.append(ResidualBlock(_local_block(cfg.block_list[0], w[0], w[0], 1, cfg.expand_list[0], cfg.fewer_norm_list[0], dtype, device), True))
        stages = [OpSequential(stage0)]
        cin = w[0]
        for s in range(1, len(w)):
            kind, fewer = cfg.block_list[s], cfg.fewer_norm_list[s]
            if kind not in ("res", "fmb", "mb", "att", "att@3"):
                raise L.OmgHipError(f"EfficientViT: block type {kind!r} is not built (the l and xl series use res, fmb, mb, att, att@3)")
            stage = [ResidualBlock(_local_block(kind if kind in ("mb", "fmb") else "mb", cin, w[s], 2, cfg.expand_list[s] * 4, fewer, dtype, device), False)]
            cin = w[s]
            for _ in range(d[s]):
                if kind in ("att", "att@3"):
                    stage.append(EfficientViTBlock(cin, cfg.qkv_dim, cfg.expand_list[s], dtype, device, scales=(3,) if kind == "att@3" else (5,),
                                                   aggreg="fused" if cfg.fused_aggreg else "gemm"))
                else:
                    stage.append(ResidualBlock(_local_block(kind, cin, cin, 1, cfg.expand_list[s], fewer, dtype, device), True))
            stages.append(OpSequential(stage))
        self.stages = nn.ModuleList(stages)


class _Neck(nn.Module):
    def __init__(self, cfg: EfficientViTSamConfig, dtype, device):
        super().__init__()
        hw = cfg.head_width
        self.input_ops = nn.ModuleList([OpSequential([ConvLayer(cfg.width_list[f], hw, "pw", 1, False, True, False, dtype, device)]) for f in cfg.neck_fids])
        self.middle = OpSequential([ResidualBlock(_local_block(cfg.neck_middle, hw, hw, 1, cfg.neck_expand, False, dtype, device), True)
                                    for _ in range(cfg.head_depth)])
        self.output_ops = nn.ModuleList([OpSequential([ConvLayer(hw, cfg.out_dim, "pw", 1, True, False, False, dtype, device)])])


class _LayerNorm(nn.Module):
    def __init__(self, c, dtype, device):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c, dtype=dtype, device=device), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(c, dtype=dtype, device=device), requires_grad=False)
        self.eps = 1e-5


# ---------------------------------------------------------------------------------------------- the encoder
class EfficientViTSamImageEncoder(PackedCache):
    def __init__(self, variant: Union[str, EfficientViTSamConfig] = "l0", dtype=torch.float16, device=None):
        super().__init__()
        cfg = variant if isinstance(variant, EfficientViTSamConfig) else EfficientViTSamConfig.variant(variant)
        n = len(cfg.width_list)
        if not (len(cfg.depth_list) == len(cfg.block_list) == len(cfg.expand_list) == len(cfg.fewer_norm_list) == n):
            raise L.OmgHipError("EfficientViTSamConfig: width, depth, block, expand and fewer_norm lists differ in length")
        self.cfg = cfg
        self.backbone = _Backbone(cfg, dtype, device)
        self.neck = _Neck(cfg, dtype, device)
        self.norm = _LayerNorm(cfg.out_dim, dtype, device)

    # ------------------------------------------------------------------ packed (BatchNorm-folded) weights, built once per layer
    def _pk(self, layer: ConvLayer):
        pk = super()._pk()
        p = pk.get(id(layer))
        if p is None:
            p = pk[id(layer)] = layer.packed()
        return p

    # ------------------------------------------------------------------ blocks on NHWC tensors
    def _c3(self, layer, x, residual=None):
        w, b = self._pk(layer)
        return ops.conv3x3_nhwc_act(x, w, stride=layer.stride, bias=b, gelu=layer.act, residual=residual)

    def _pw(self, layer, x, residual=None):
        w, b = self._pk(layer)
        B, H, W, C = x.shape
        y = ops.gemm(x.view(B * H * W, C), w, bias=b, residual=residual.view(B * H * W, -1) if residual is not None else None)
        return y.view(B, H, W, layer.cout)

    def _block(self, blk, x, shortcut: bool):
        res = x if shortcut else None
        if isinstance(blk, ResBlock):
            return self._c3(blk.conv2, self._c3(blk.conv1, x), res)
        if isinstance(blk, FusedMBConv):
            return self._pw(blk.point_conv, self._c3(blk.spatial_conv, x), res)
        if isinstance(blk, MBConv):
            B, H, W, _ = x.shape
            h = self._pw(blk.inverted_conv, x)                              # pre-activation; its GELU is applied by the depthwise kernel's loads
            dw = blk.depth_conv
            w, b = self._pk(dw)
            t = ops.dwconv3x3_act(h.view(B * H * W, -1), w, B, H, W, stride=dw.stride, bias=b, gelu=True, gelu_in=True)
            Ho, Wo = (H - 1) // dw.stride + 1, (W - 1) // dw.stride + 1
            return self._pw(blk.point_conv, t.view(B, Ho, Wo, -1), res)
        if isinstance(blk, LiteMLA):
            return blk.forward_nhwc(x, residual=shortcut)
        raise L.OmgHipError(f"EfficientViT: no kernel path for {type(blk).__name__}")

    def _op(self, op, x):
        if isinstance(op, ConvLayer):
            return self._c3(op, x) if op.kind == "c3" else self._pw(op, x)
        if isinstance(op, EfficientViTBlock):
            x = self._block(op.context_module.main, x, True)
            return self._block(op.local_module.main, x, True)
        return self._block(op.main, x, op.has_shortcut)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward_features(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """NCHW input -> {"stage0" .. "stageN", "neck_mid", "neck", "out"}: NHWC tensors ("out" is the embedding before the final permute)."""
        if not x.is_cuda:
            raise L.OmgHipError("EfficientViTSamImageEncoder needs its input on the MI355X (cuda/hip device); there is no CPU fallback")
        dt = self.norm.weight.dtype
        if x.dtype != dt or x.dim() != 4 or x.shape[1] != 3:
            raise L.OmgHipError(f"EfficientViTSamImageEncoder: input must be [B, 3, H, W] in {dt}")
        cfg = self.cfg
        feats: Dict[str, torch.Tensor] = {}
        h = x.permute(0, 2, 3, 1).contiguous()
        for s, stage in enumerate(self.backbone.stages):
            for op in stage.op_list:
                h = self._op(op, h)
            feats[f"stage{s}"] = h
        # neck: 1x1 convolution of each input, resized to the grid and summed; an input already on the grid is the sum's first term
        G = cfg.grid
        B = x.shape[0]
        on_grid = [i for i, f in enumerate(cfg.neck_fids) if feats[f"stage{f}"].shape[1:3] == (G, G)]
        acc: Optional[torch.Tensor] = None
        for i in on_grid:
            acc = self._pw(self.neck.input_ops[i].op_list[0], feats[f"stage{cfg.neck_fids[i]}"], residual=acc)
        for i, f in enumerate(cfg.neck_fids):
            if i in on_grid:
                continue
            t = self._pw(self.neck.input_ops[i].op_list[0], feats[f"stage{f}"])
            if acc is None:
                acc = ops.upsample_add_nhwc(t, torch.empty((B, G, G, cfg.head_width), dtype=dt, device=x.device), accumulate=False)
            else:
                ops.upsample_add_nhwc(t, acc, accumulate=True)
        h = acc
        for op in self.neck.middle.op_list:
            h = self._op(op, h)
        feats["neck_mid"] = h
        h = self._pw(self.neck.output_ops[0].op_list[0], h)
        feats["neck"] = h
        feats["out"] = ops.layernorm(h, self.norm.weight.data, self.norm.bias.data, self.norm.eps)
        return feats

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (B, 3, H, W), 16-bit, resized / normalised / padded -> the image embedding (B, out_dim, grid, grid) (a permuted view of the NHWC result)."""
        return self.forward_features(x)["out"].permute(0, 3, 1, 2)
