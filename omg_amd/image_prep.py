"""Pillow's 8-bit ``Image.resize`` on the device, with the normalise / pad / permute / cast of a preprocessor in the same launches.

``Image.resize(size, resample)`` on an RGB image (default ``box`` and ``reducing_gap``) is two passes of fixed-point arithmetic: per axis
and output index a window ``[xmin, xmin + n)`` of the input and ``n`` 22-bit integer coefficients, computed in float64 from the sizes
alone; a pass is ``clip((2^21 + sum pixel * coeff) >> 22, 0, 255)`` in 32-bit integers, the horizontal pass first and rounded to 8 bits,
and a pass whose axis keeps its size is skipped.  :func:`resize_tables` computes the windows and coefficients, :func:`resize_reference`
is the numpy model of the two passes (the CPU tests hold it against Pillow itself), and ``ops.image_prep`` runs the passes on the
tables (omg_image_resize_h, omg_image_resize_v: csrc/image_prep.hip) — the kernels are filter-agnostic.

What follows a resize in every preprocessor here is a function of the 8-bit value and the channel alone, so it is a ``[3, 256]`` lookup
table built once WITH THE HOST PATH'S OWN EXPRESSION (``lut_*`` below): the vertical pass looks its 8-bit result up and stores the
planar, padded tensor of the network's dtype, bit-equal to the host path by construction.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

__all__ = ["BILINEAR", "BICUBIC", "resize_tables", "resize_reference", "device_tables", "to_uint8_hwc", "lut_unit_mean_std", "lut_sam",
           "lut_numpy_rescale_mean_std"]

BILINEAR, BICUBIC = 2, 3                      # PIL.Image.BILINEAR / BICUBIC
_NAMES = {0: "NEAREST", 1: "LANCZOS", 2: "BILINEAR", 3: "BICUBIC", 4: "BOX", 5: "HAMMING"}
PRECISION_BITS = 22


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTERS = {BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0)}


def check_resample(resample) -> int:
    r = int(resample)
    if r not in _FILTERS:
        raise ValueError(f"image_prep: resample {resample} ({_NAMES.get(r, 'unknown')}) is not built; BILINEAR (2) or BICUBIC (3)")
    return r


_HOST: Dict[tuple, Tuple[np.ndarray, np.ndarray]] = {}
_DEVICE: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def resize_tables(in_size: int, out_size: int, resample: int) -> Tuple[np.ndarray, np.ndarray]:
    """One axis: int32 ``bounds [out, 2]`` (first input index, number of taps) and ``coeffs [out, ksize]`` (22-bit fixed point, zeros
    behind a row's taps), in float64 as Pillow's precompute_coeffs and normalize_coeffs_8bpc."""
    r = check_resample(resample)
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"image_prep: sizes {in_size} -> {out_size}")
    key = (in_size, out_size, r)
    if key in _HOST:
        return _HOST[key]
    filt, S = _FILTERS[r]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = S * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((x + xmin - center + 0.5) / filterscale) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            coeffs[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    _HOST[key] = (bounds, coeffs)
    return bounds, coeffs


def _pass(a: np.ndarray, axis: int, out_size: int, resample: int) -> np.ndarray:
    """One pass along ``axis`` of a uint8 array, in int32 as ImagingResampleHorizontal_8bpc / Vertical."""
    bounds, coeffs = resize_tables(a.shape[axis], out_size, resample)
    src = np.moveaxis(a, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for xx in range(out_size):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        k = coeffs[xx, :n].reshape((n,) + (1,) * (src.ndim - 1))
        ss = (1 << (PRECISION_BITS - 1)) + (src[xmin:xmin + n] * k).sum(axis=0, dtype=np.int32)
        out[xx] = np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_reference(array: np.ndarray, size: Sequence[int], resample: int) -> np.ndarray:
    """``np.asarray(Image.fromarray(array).resize((ow, oh), resample))`` for a uint8 [H, W, C] array, without Pillow."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError(f"resize_reference takes a uint8 [H, W, C] array, got {a.dtype} {a.shape}")
    ow, oh = int(size[0]), int(size[1])
    check_resample(resample)
    if ow != a.shape[1]:
        a = _pass(a, 1, ow, resample)
    if oh != a.shape[0]:
        a = _pass(a, 0, oh, resample)
    return np.ascontiguousarray(a)


def device_tables(in_size: int, out_size: int, resample: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`resize_tables` on ``device``, uploaded once per (in, out, resample, device).  A graph capture cannot upload: the first,
    uncaptured call of a preprocessor (the warm-up every capture here has) puts its tables in place."""
    device = torch.device(device)
    key = (int(in_size), int(out_size), int(resample), device.type, device.index if device.index is not None else torch.cuda.current_device())
    t = _DEVICE.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"image_prep: the resize tables {in_size} -> {out_size} are not on the device yet and a graph capture cannot "
                               "upload them; run the call once before capturing it")
        bounds, coeffs = resize_tables(in_size, out_size, resample)
        t = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(coeffs.copy()).to(device))
        _DEVICE[key] = t
    return t


def to_uint8_hwc(images: torch.Tensor) -> torch.Tensor:
    """The pipeline's ``output_type="pt"`` result ([n, 3, H, W] or [3, H, W], values in [0, 1]) -> uint8 [n, H, W, 3] / [H, W, 3] on
    the tensor's device: ``(x.float() * 255).round()``, the float32 arithmetic of the pipeline's own ``(x * 255).round().astype("uint8")``."""
    if images.dim() not in (3, 4) or images.shape[-3] != 3:
        raise ValueError(f"to_uint8_hwc takes [n, 3, H, W] or [3, H, W], got {tuple(images.shape)}")
    x = (images.float() * 255).round().to(torch.uint8)
    return x.movedim(-3, -1).contiguous()


# ---------------------------------------------------------------------------------------------- lookup tables [3, 256]
def _u8() -> torch.Tensor:
    return torch.arange(256, dtype=torch.int32).to(torch.uint8)


def lut_unit_mean_std(mean: Sequence[float], std: Sequence[float], dtype: torch.dtype, device) -> torch.Tensor:
    """``ToTensor`` + ``Normalize(mean, std)`` of a host preprocessor: ``((u8.float() / 255) - mean) / std`` in fp32 on the host, then
    ``.to(dtype)``."""
    m = torch.tensor(list(mean), dtype=torch.float32)[:, None]
    s = torch.tensor(list(std), dtype=torch.float32)[:, None]
    x = _u8().float().div(255)[None].expand(3, -1)
    return ((x - m) / s).to(dtype).contiguous().to(device)


def lut_sam(pixel_mean: torch.Tensor, pixel_std: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``Sam.preprocess``: ``(u8.float() - pixel_mean) / pixel_std`` with the model's own buffers, on their device, then ``.to(dtype)``."""
    x = _u8().to(pixel_mean.device).float()[None].expand(3, -1)
    return ((x - pixel_mean.float().view(3, 1)) / pixel_std.float().view(3, 1)).to(dtype).contiguous()


def lut_numpy_rescale_mean_std(rescale, mean, std, dtype: torch.dtype, device) -> torch.Tensor:
    """The numpy lines of ``DPTImageProcessor``: ``a = u8.astype(float32)``, ``a * float32(rescale)`` (or not), ``(a - mean) / std`` (or
    not) in float32; ``rescale`` / ``mean`` None = that step is off."""
    a = np.broadcast_to(np.arange(256, dtype=np.uint8).astype(np.float32)[:, None], (256, 3))
    if rescale is not None:
        a = a * np.float32(rescale)
    if mean is not None:
        a = (a - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(dtype).contiguous().to(device)
