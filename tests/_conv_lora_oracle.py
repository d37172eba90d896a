"""Float64 reference of LoRA on a convolution (PEFT ``lora.Conv2d``, LyCORIS "LoCon"), shared by tests/test_conv_lora.py (CPU) and
tests/test_conv_lora_gpu.py.  A wrapped ``Conv2d(Cin, Cout, k, stride, padding)`` computes

    y = conv(x; W) + s * B(A(x)),    A: k x k conv Cin -> r with the base layer's stride and padding,  B: 1x1 conv r -> Cout

whose merged form is ``W' = W + s * sum_r B[o, r] * A[r, i, ky, kx]``.  Nothing here calls the product.
"""
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F


def delta_weight(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """``dW[o, i, ky, kx] = sum_r B[o, r] A[r, i, ky, kx]`` in float64; B is ``[Cout, r]`` or ``[Cout, r, 1, 1]``."""
    A, B = A.double(), B.double().reshape(B.shape[0], -1)
    return torch.einsum("or,rikl->oikl", B, A)


def unmerged(x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, stride: int = 1, padding: int = 0) -> torch.Tensor:
    """``B(A(x))`` on NCHW ``x`` in float64, written as im2col + two matrix products (no conv call)."""
    x, A, B = x.double(), A.double(), B.double().reshape(B.shape[0], -1)
    n, _, h, w = x.shape
    k = A.shape[-1]
    ho, wo = (h + 2 * padding - k) // stride + 1, (w + 2 * padding - k) // stride + 1
    cols = F.unfold(x, k, padding=padding, stride=stride)                 # [n, Cin*k*k, ho*wo], rows in (ci, ky, kx) order
    t = A.reshape(A.shape[0], -1) @ cols                                  # [n, r, ho*wo]
    return (B @ t).reshape(n, B.shape[0], ho, wo)


def merged_weight(W: torch.Tensor, pairs: Sequence[Tuple[torch.Tensor, torch.Tensor, float]]) -> torch.Tensor:
    """``W + sum_a s_a * B_a A_a`` in float64; ``pairs`` = [(A, B, s)]."""
    out = W.double().clone()
    for A, B, s in pairs:
        out += float(s) * delta_weight(A, B)
    return out


def merged_state_dict(sd: Dict[str, torch.Tensor], conv_lora: Dict[str, Tuple[torch.Tensor, torch.Tensor]], scale: float,
                      dtype: Optional[torch.dtype] = None) -> Dict[str, torch.Tensor]:
    """A copy of the oracle state dict ``sd`` whose conv weights carry ``scale * B A`` (fp32 merge; rounded once through ``dtype`` when
    given, as the engine's merged mode stores it)."""
    out = dict(sd)
    for key, (A, B) in conv_lora.items():
        w = merged_weight(sd[key + ".weight"], [(A, B, scale)]).float()
        out[key + ".weight"] = w.to(dtype).float() if dtype is not None else w
    return out


def conv_nhwc(x1: torch.Tensor, W: torch.Tensor, *, x2: Optional[torch.Tensor] = None, stride: int = 1, upsample: bool = False,
              bias=None, group_bias=None, residual=None, out_scale: float = 1.0, silu: bool = False,
              extra: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Float64 model of ``ops.conv2d`` on CPU tensors: NHWC in / out, OIHW weight ``W`` over the concat of ``x1`` and ``x2``, pad 1 for
    3x3, nearest-2x upsample first; ``extra`` (NHWC) joins the accumulator before the epilogue
    ``act(acc + bias + group_bias) * out_scale + residual``."""
    x = x1.double() if x2 is None else torch.cat([x1.double(), x2.double()], dim=-1)
    x = x.permute(0, 3, 1, 2)
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, W.double(), stride=stride, padding=1 if W.shape[-1] == 3 else 0).permute(0, 2, 3, 1)
    if extra is not None:
        y = y + extra.double()
    if bias is not None:
        y = y + bias.double()
    if group_bias is not None:
        y = y + group_bias.double()[:, None, None, :]
    if silu:
        y = F.silu(y)
    y = y * out_scale
    if residual is not None:
        y = y + residual.double()
    return y


def lora_nhwc(x1: torch.Tensor, A: torch.Tensor, B: torch.Tensor, *, x2=None, stride: int = 1, upsample: bool = False) -> torch.Tensor:
    """``B(A(x))`` (NHWC float64) with the base layer's stride / padding / upsample: the term PEFT adds."""
    x = x1.double() if x2 is None else torch.cat([x1.double(), x2.double()], dim=-1)
    x = x.permute(0, 3, 1, 2)
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return unmerged(x, A, B, stride=stride, padding=1 if A.shape[-1] == 3 else 0).permute(0, 2, 3, 1)


def conv_targets(ocfg) -> list:
    """The conv LoRA targets of the oracle's parameter table: every 4-D weight but conv_in / conv_out."""
    from oracle import unet as ou
    return [k[:-len(".weight")] for k, shp in ou.param_shapes(ocfg).items()
            if k.endswith(".weight") and len(shp) == 4 and not k.startswith(("conv_in", "conv_out"))]


def make_conv_lora(ocfg, names, rank: int, seed: int, dtype) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """Synthetic conv adapters in the style of oracle.unet.make_lora: A [r, Cin, k, k] ~ N(0, 1 / fan_in), B [Cout, r] ~ N(0, 1e-2), rounded through ``dtype``."""
    from oracle import unet as ou
    shapes = ou.param_shapes(ocfg)
    g = torch.Generator().manual_seed(seed)
    w = {}
    for k in names:
        o, i, kh, kw = shapes[k + ".weight"]
        A = (torch.randn(rank, i, kh, kw, generator=g) * (i * kh * kw) ** -0.5).to(dtype).float()
        Bm = (torch.randn(o, rank, generator=g) * 0.1).to(dtype).float()
        w[k] = (A, Bm)
    return w
