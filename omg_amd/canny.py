"""The demos' Canny edge condition (``get_cannyedge``, gradio_demo/app.py:332: ``cv2.Canny(np.array(image), 100, 200)``, three equal
channels) on HIP kernels, and the arithmetic as a numpy model.

The model (:func:`nms_reference`, :func:`hysteresis_reference`, :func:`canny_reference`) is ``cv2.Canny(image, threshold1, threshold2)``
at its defaults (``apertureSize=3``, ``L2gradient=False``) written from OpenCV's published algorithm.  OpenCV is not installed where this
package is developed, so the model is NOT pinned against it: tests/test_canny.py compares the two wherever ``cv2`` can be imported and
skips elsewhere.  What is pinned: two hand-derived images, the gradients against ``scipy.ndimage.correlate`` and the hysteresis against
``scipy.ndimage.label``; the kernels (csrc/canny.hip) equal the model bit for bit.

Integers throughout:

1. thresholds: swapped when ``threshold1 > threshold2``; ``low = floor(threshold1)``, ``high = floor(threshold2)``.
2. per channel the 3x3 Sobel ``dx`` (columns ``[-1 0 1]``, rows weighted ``1 2 1``) and ``dy`` (its transpose) on the replicated border;
   ``mag = |dx| + |dy|`` (at most 2040).
3. with three channels a pixel takes ``dx, dy, mag`` of the channel with the largest ``mag``, the lowest index on a tie.
4. non-maximum suppression, the magnitude outside the image being 0: a pixel with ``mag > low`` is a candidate; with ``x = |dx|``,
   ``y = |dy| << 15``, ``t22 = x * 13573``, ``t67 = t22 + (x << 16)`` it is kept when

       y < t22                       mag > left and mag >= right
       y > t67                       mag > up and mag >= down
       else, (dx ^ dy) >= 0          mag > up-left and mag > down-right
       else                          mag > up-right and mag > down-left

5. the state map (this package's coding, uint8): 0 not an edge, 1 kept and ``mag <= high`` (weak), 2 kept and ``mag > high`` (strong).
6. hysteresis: 255 on every pixel of state 1 or 2 whose 8-connected component of non-zero states holds a state-2 pixel, 0 elsewhere — a
   function of the map alone, whatever order an implementation visits it in.

The public layer: :func:`Canny` (cv2's positional signature; numpy in, numpy out through the device; cuda tensor in, cuda tensor out)
and :func:`canny_condition` (the demos' ``get_cannyedge``).  ``compat.install()`` gives its ``cv2`` stand-in this ``Canny``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

MAG_MAX = 2040          # 4 * 255 + 4 * 255


def thresholds(threshold1, threshold2) -> Tuple[int, int]:
    """``(low, high)`` as the kernels take them: swapped if need be, floored, and clamped into [0, MAG_MAX + 1] — a magnitude is an
    integer in [0, MAG_MAX] and a pixel of magnitude 0 is never kept, so the clamp changes no result."""
    t1, t2 = float(threshold1), float(threshold2)
    if math.isnan(t1) or math.isnan(t2):
        raise ValueError(f"Canny: thresholds ({threshold1}, {threshold2}) hold a NaN")
    if t1 > t2:
        t1, t2 = t2, t1
    clamp = lambda t: int(min(max(math.floor(t), 0), MAG_MAX + 1))
    return clamp(t1), clamp(t2)


def _check_image(image: np.ndarray) -> np.ndarray:
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.size == 0:
        raise ValueError(f"Canny takes a uint8 [H, W] or [H, W, C] image with C of 1 or 3, got {a.dtype} {a.shape}")
    return a[:, :, None] if a.ndim == 2 else a


def sobel_reference(image: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(dx, dy)`` int32 ``[H, W, C]`` of a uint8 ``[H, W]`` / ``[H, W, C]`` image: 3x3 Sobel on the replicated border."""
    a = _check_image(image).astype(np.int32)
    H, W, _ = a.shape
    p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge")
    win = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    dx = (win(-1, 1) + 2 * win(0, 1) + win(1, 1)) - (win(-1, -1) + 2 * win(0, -1) + win(1, -1))
    dy = (win(1, -1) + 2 * win(1, 0) + win(1, 1)) - (win(-1, -1) + 2 * win(-1, 0) + win(-1, 1))
    return dx, dy


def nms_reference(image: np.ndarray, low: int, high: int) -> np.ndarray:
    """Steps 2-5: uint8 ``[H, W]`` / ``[H, W, C]`` -> the uint8 state map ``[H, W]`` for integer thresholds ``low <= high``."""
    dx, dy = sobel_reference(image)
    H, W, C = dx.shape
    mag = np.abs(dx) + np.abs(dy)
    ch = np.argmax(mag, axis=2)                     # the first maximum: the lowest channel on a tie
    pick = lambda v: np.take_along_axis(v, ch[:, :, None], axis=2)[:, :, 0]
    dx, dy, mag = pick(dx), pick(dy), pick(mag)
    assert mag.max() <= MAG_MAX
    m = np.pad(mag, 1)                              # 0 outside the image
    nb = lambda oy, ox: m[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    cand = mag > low
    assert not (cand & (mag > 0) & ((y == t22) | (y == t67))).any()      # 13573 and 79109 are odd
    horiz = y < t22
    vert = ~horiz & (y > t67)
    diag = ~horiz & ~vert
    same = (dx ^ dy) >= 0
    keep = np.where(horiz, (mag > nb(0, -1)) & (mag >= nb(0, 1)),
           np.where(vert, (mag > nb(-1, 0)) & (mag >= nb(1, 0)),
           np.where(diag & same, (mag > nb(-1, -1)) & (mag > nb(1, 1)),
                    (mag > nb(-1, 1)) & (mag > nb(1, -1)))))
    keep &= cand
    return np.where(keep, np.where(mag > high, 2, 1), 0).astype(np.uint8)


def hysteresis_reference(state: np.ndarray) -> np.ndarray:
    """Step 6: uint8 state map ``[H, W]`` -> uint8 edges ``[H, W]`` (0 / 255), by a stack flood fill from the strong pixels."""
    s = np.asarray(state)
    if s.ndim != 2 or s.dtype != np.uint8 or (s.size and s.max() > 2):
        raise ValueError(f"hysteresis_reference takes a uint8 [H, W] state map of 0, 1 and 2, got {s.dtype} {s.shape}")
    H, W = s.shape
    out = np.zeros((H, W), dtype=np.uint8)
    stack = [(int(y), int(x)) for y, x in zip(*np.nonzero(s == 2))]
    for y, x in stack:
        out[y, x] = 255
    while stack:
        y, x = stack.pop()
        for yy in range(max(y - 1, 0), min(y + 2, H)):
            for xx in range(max(x - 1, 0), min(x + 2, W)):
                if s[yy, xx] and not out[yy, xx]:
                    out[yy, xx] = 255
                    stack.append((yy, xx))
    return out


def canny_reference(image: np.ndarray, threshold1, threshold2) -> np.ndarray:
    """The whole model: uint8 ``[H, W]`` / ``[H, W, C]`` -> uint8 edges ``[H, W]`` (0 / 255)."""
    low, high = thresholds(threshold1, threshold2)
    return hysteresis_reference(nms_reference(image, low, high))


# ---------------------------------------------------------------------------------------------- the public layer (HIP kernels)
def _device():
    import torch
    from . import _lib as L
    if not torch.cuda.is_available():
        raise L.OmgHipError("Canny runs on the MI355X (cuda/hip device) and none is available; omg_amd has no CPU fallback "
                            "(omg_amd.canny.canny_reference is the numpy model)")
    return torch.device("cuda", torch.cuda.current_device())


def Canny(image, threshold1, threshold2, edges=None, apertureSize=3, L2gradient=False):
    """``cv2.Canny(image, threshold1, threshold2)``: a uint8 ``[H, W]`` / ``[H, W, C]`` (C 1 or 3) image -> uint8 edges ``[H, W]`` (0 / 255).
    A numpy array goes through the device and comes back as a numpy array; a cuda tensor gives a cuda tensor.  Refused by name:
    ``apertureSize`` other than 3, ``L2gradient=True``, a preallocated ``edges``."""
    import torch
    from . import _lib as L, ops
    if edges is not None:
        raise L.OmgHipError("Canny: edges (a preallocated output) is not supported; the result is returned")
    if apertureSize != 3:
        raise L.OmgHipError(f"Canny: apertureSize={apertureSize} is not supported, only the 3x3 Sobel (apertureSize=3)")
    if L2gradient:
        raise L.OmgHipError("Canny: L2gradient=True is not supported, only the L1 magnitude |dx| + |dy| (L2gradient=False)")
    if torch.is_tensor(image):
        return ops.canny(image, threshold1, threshold2)
    try:
        a = _check_image(image)
    except ValueError as e:
        raise L.OmgHipError(str(e)) from None
    u8 = torch.from_numpy(np.ascontiguousarray(a)).to(_device())
    return ops.canny(u8, threshold1, threshold2).cpu().numpy()


def canny_condition(image, low=100, high=200, output: str = "pil", dtype=None):
    """The demos' ``get_cannyedge`` for a PIL image, a numpy array or a cuda uint8 ``[H, W, C]`` tensor: ``"pil"`` gives the three-channel
    PIL image the demos return, ``"pt"`` the planar ``[1, 3, H, W]`` tensor of 0 and 1 on the device (``dtype``: float16, bfloat16 or
    float32, the default) — what ``prepare_image`` makes of that PIL image, so a ControlNet takes it as it is."""
    import torch
    from . import _lib as L, ops
    if output not in ("pil", "pt"):
        raise L.OmgHipError(f"canny_condition: output={output!r}, expected 'pil' or 'pt'")
    if output == "pil" and dtype is not None:
        raise L.OmgHipError("canny_condition: dtype goes with output='pt'")
    if torch.is_tensor(image):
        u8 = image
    else:
        try:
            a = _check_image(np.array(image))
        except ValueError as e:
            raise L.OmgHipError(str(e)) from None
        u8 = torch.from_numpy(np.ascontiguousarray(a)).to(_device())
    if u8.dim() == 4:
        raise L.OmgHipError(f"canny_condition takes one image, got a batch {tuple(u8.shape)}")
    if output == "pt":
        return ops.canny(u8, low, high, out_dtype=torch.float32 if dtype is None else dtype)[None]
    from PIL import Image
    return Image.fromarray(ops.canny(u8, low, high, channels=3).cpu().numpy())
