"""Normalisation kernels on badly conditioned inputs, and the small entry points nobody tested directly (-m gpu).

Every reference is a float64 torch-CPU computation on the STORED inputs (the values after rounding to the storage type).

1. GroupNorm with |mean| >> std (one chunk, many ragged chunks, two vectors per lane, the fused concat, one group), per-group
   and per-sample offsets, an outlier first pixel, a constant tensor, a spread far below eps, fp16 near the top of its range.
   16-bit storage: the suite's own tolerance (TOL / close of tests/test_kernels_gpu.py, scale = 2).  fp32 storage: no number of
   our own — torch's fp32 CPU F.group_norm is measured against the float64 reference on the same input and the kernel gets
   max(2e-5, 4 x that) in max-abs error (2e-5: the bound of the existing fp32 check; 4: another summation order and fma
   contraction; torch folds x * scale + shift, which cancels like a naive apply pass, so it is a generous yardstick).
2. omg_groupnorm_mx8 stays the bit-exact quantisation of omg_groupnorm's output on such inputs.
3. LayerNorm: the same families, one to four vectors per lane, a ragged last vector row, row counts off the four rows per
   block, strided rows, the MX-fp8 form, argument validation.
4. omg_softmax_rows: the text encoder's causal -30000 mask, constant rows, +-65504, a dominant entry, columns around the block
   width, untouched padding.
5. omg_add_inplace, omg_gather_step, omg_scale_model_input bit for bit; omg_fuse_cfg_step against a float64 restatement of the
   contract in include/omg_hip.h.

fp32 GroupNorm on the MI355X (B = 2, eps = 1e-6, worst of silu off / on; `limit` = max(2e-5, 4 x torch-fp32)).  The statistics
are sums shifted by a per-channel pivot and merged as (mean, M2).  Last column: the same case on the plain fp32
sum x / sum x^2 statistics they replaced, which failed 96 of these 114 cases, 24 of the 16-bit ones (256/1, -256/1, per-group,
per-sample: up to 0.05 where 0.004 is allowed) and both fp16 cases of section 2.

       family | HW x C           | torch-fp32 | this kernel | limit   | sum x / sum x^2 kernel
        0.5/2 | 64 x 320  G=32   |    1.4e-06 |     1.3e-06 | 2.0e-05 | 1.5e-06
        0.5/2 | 1000 x 320  G=32 |    1.5e-06 |     1.4e-06 | 2.0e-05 | 1.7e-06
        0.5/2 | 4096 x 128  G=32 |    1.4e-06 |     2.0e-06 | 2.0e-05 | 1.5e-06
        0.5/2 | 64 x 2560 G=32   |    1.6e-06 |     1.5e-06 | 2.0e-05 | 3.5e-06
        0.5/2 | 256 x 960  G=32  |    1.5e-06 |     1.9e-06 | 2.0e-05 | 3.0e-06
        0.5/2 | 300 x 64   G=1   |    1.1e-06 |     1.2e-06 | 2.0e-05 | 2.8e-06
         16/1 | 64 x 320  G=32   |    4.3e-06 |     3.0e-06 | 2.0e-05 | 7.0e-04
         16/1 | 1000 x 320  G=32 |    6.9e-06 |     3.7e-06 | 2.8e-05 | 1.6e-04
         16/1 | 4096 x 128  G=32 |    5.3e-06 |     2.7e-06 | 2.1e-05 | 1.5e-04
         16/1 | 64 x 2560 G=32   |    5.4e-06 |     3.0e-06 | 2.2e-05 | 3.8e-04
         16/1 | 256 x 960  G=32  |    7.3e-06 |     3.2e-06 | 2.9e-05 | 3.0e-04
         16/1 | 300 x 64   G=1   |    2.0e-06 |     2.0e-06 | 2.0e-05 | 3.6e-03
         64/1 | 64 x 320  G=32   |    2.4e-05 |     1.1e-05 | 9.8e-05 | 1.1e-02
         64/1 | 1000 x 320  G=32 |    2.4e-05 |     1.4e-05 | 9.7e-05 | 2.4e-03
         64/1 | 4096 x 128  G=32 |    1.6e-05 |     6.9e-06 | 6.5e-05 | 2.5e-03
         64/1 | 64 x 2560 G=32   |    2.6e-05 |     1.3e-05 | 1.1e-04 | 5.1e-03
         64/1 | 256 x 960  G=32  |    2.2e-05 |     1.1e-05 | 8.6e-05 | 2.5e-03
         64/1 | 300 x 64   G=1   |    1.3e-05 |     1.5e-05 | 5.3e-05 | 7.4e-02
        256/1 | 64 x 320  G=32   |    1.2e-04 |     3.2e-05 | 4.8e-04 | 1.2e-01
        256/1 | 1000 x 320  G=32 |    1.3e-04 |     4.3e-05 | 5.1e-04 | 7.1e-02
        256/1 | 4096 x 128  G=32 |    1.0e-04 |     3.6e-05 | 4.1e-04 | 5.5e-02
        256/1 | 64 x 2560 G=32   |    1.3e-04 |     3.7e-05 | 5.2e-04 | 5.2e-02
        256/1 | 256 x 960  G=32  |    1.1e-04 |     5.2e-05 | 4.6e-04 | 5.0e-02
        256/1 | 300 x 64   G=1   |    5.9e-05 |     1.5e-05 | 2.4e-04 | 6.8e-01
       1000/1 | 64 x 320  G=32   |    2.6e-04 |     8.1e-05 | 1.0e-03 | 9.3e+00
       1000/1 | 1000 x 320  G=32 |    2.6e-04 |     1.1e-04 | 1.0e-03 | 1.0e+00
       1000/1 | 4096 x 128  G=32 |    2.1e-04 |     8.0e-05 | 8.3e-04 | 6.9e-01
       1000/1 | 64 x 2560 G=32   |    3.0e-04 |     1.2e-04 | 1.2e-03 | 1.7e+00
       1000/1 | 256 x 960  G=32  |    2.7e-04 |     9.8e-05 | 1.1e-03 | 7.7e-01
       1000/1 | 300 x 64   G=1   |    1.9e-04 |     7.6e-05 | 7.7e-04 | 4.9e+00
      100/0.1 | 64 x 320  G=32   |    4.2e-04 |     1.4e-04 | 1.7e-03 | 2.7e+00
      100/0.1 | 1000 x 320  G=32 |    3.5e-04 |     1.0e-04 | 1.4e-03 | 7.8e-01
      100/0.1 | 4096 x 128  G=32 |    3.2e-04 |     1.1e-04 | 1.3e-03 | 5.1e-01
      100/0.1 | 64 x 2560 G=32   |    2.9e-04 |     1.1e-04 | 1.2e-03 | 1.0e+00
      100/0.1 | 256 x 960  G=32  |    3.1e-04 |     1.4e-04 | 1.2e-03 | 9.5e-01
      100/0.1 | 300 x 64   G=1   |    2.1e-04 |     7.5e-05 | 8.4e-04 | 1.3e+01
       4000/2 | 64 x 320  G=32   |    7.0e-04 |     2.3e-04 | 2.8e-03 | 1.5e+04
       4000/2 | 1000 x 320  G=32 |    4.3e-04 |     1.3e-04 | 1.7e-03 | 1.5e+01
       4000/2 | 4096 x 128  G=32 |    4.4e-04 |     1.8e-04 | 1.8e-03 | 4.4e+00
       4000/2 | 64 x 2560 G=32   |    4.6e-04 |     2.0e-04 | 1.8e-03 | 2.6e+01
       4000/2 | 256 x 960  G=32  |    7.0e-04 |     1.6e-04 | 2.8e-03 | 1.3e+01
       4000/2 | 300 x 64   G=1   |    5.7e-04 |     1.7e-04 | 2.3e-03 | 2.3e+04
        -16/1 | 64 x 320  G=32   |    5.2e-06 |     2.8e-06 | 2.1e-05 | 7.9e-04
        -16/1 | 1000 x 320  G=32 |    4.9e-06 |     3.0e-06 | 2.0e-05 | 1.8e-04
        -16/1 | 4096 x 128  G=32 |    1.4e-05 |     3.3e-06 | 5.4e-05 | 2.6e-04
        -16/1 | 64 x 2560 G=32   |    8.4e-06 |     3.2e-06 | 3.3e-05 | 3.9e-04
        -16/1 | 256 x 960  G=32  |    7.6e-06 |     3.9e-06 | 3.0e-05 | 2.0e-04
        -16/1 | 300 x 64   G=1   |    4.2e-06 |     3.2e-06 | 2.0e-05 | 1.9e-03
        -64/1 | 64 x 320  G=32   |    1.8e-05 |     1.4e-05 | 7.3e-05 | 9.7e-03
        -64/1 | 1000 x 320  G=32 |    2.1e-05 |     1.1e-05 | 8.2e-05 | 2.5e-03
        -64/1 | 4096 x 128  G=32 |    3.5e-05 |     1.1e-05 | 1.4e-04 | 2.6e-03
        -64/1 | 64 x 2560 G=32   |    2.8e-05 |     1.3e-05 | 1.1e-04 | 4.2e-03
        -64/1 | 256 x 960  G=32  |    1.7e-05 |     1.0e-05 | 6.7e-05 | 3.4e-03
        -64/1 | 300 x 64   G=1   |    1.3e-05 |     1.2e-05 | 5.1e-05 | 3.4e-02
       -256/1 | 64 x 320  G=32   |    1.2e-04 |     3.4e-05 | 4.8e-04 | 1.2e-01
       -256/1 | 1000 x 320  G=32 |    7.5e-05 |     4.1e-05 | 3.0e-04 | 3.7e-02
       -256/1 | 4096 x 128  G=32 |    1.2e-04 |     5.7e-05 | 4.6e-04 | 4.5e-02
       -256/1 | 64 x 2560 G=32   |    1.0e-04 |     3.7e-05 | 4.2e-04 | 7.3e-02
       -256/1 | 256 x 960  G=32  |    8.0e-05 |     4.0e-05 | 3.2e-04 | 5.6e-02
       -256/1 | 300 x 64   G=1   |    9.6e-05 |     5.0e-05 | 3.8e-04 | 3.9e-01
      -1000/1 | 64 x 320  G=32   |    3.5e-04 |     8.1e-05 | 1.4e-03 | 2.3e+00
      -1000/1 | 1000 x 320  G=32 |    2.7e-04 |     1.1e-04 | 1.1e-03 | 1.2e+00
      -1000/1 | 4096 x 128  G=32 |    1.5e-04 |     7.3e-05 | 6.1e-04 | 6.9e-01
      -1000/1 | 64 x 2560 G=32   |    2.5e-04 |     1.2e-04 | 1.0e-03 | 1.3e+00
      -1000/1 | 256 x 960  G=32  |    2.8e-04 |     9.8e-05 | 1.1e-03 | 1.1e+00
      -1000/1 | 300 x 64   G=1   |    2.1e-04 |     7.6e-05 | 8.2e-04 | 1.2e+04
     -100/0.1 | 64 x 320  G=32   |    3.4e-04 |     1.4e-04 | 1.4e-03 | 4.2e+00
     -100/0.1 | 1000 x 320  G=32 |    2.3e-04 |     1.0e-04 | 9.3e-04 | 9.5e-01
     -100/0.1 | 4096 x 128  G=32 |    3.3e-04 |     1.1e-04 | 1.3e-03 | 8.8e-01
     -100/0.1 | 64 x 2560 G=32   |    3.3e-04 |     1.1e-04 | 1.3e-03 | 9.9e-01
     -100/0.1 | 256 x 960  G=32  |    3.1e-04 |     1.5e-04 | 1.2e-03 | 9.0e-01
     -100/0.1 | 300 x 64   G=1   |    1.8e-04 |     7.5e-05 | 7.1e-04 | 7.0e+00
      -4000/2 | 64 x 320  G=32   |    6.8e-04 |     2.3e-04 | 2.7e-03 | 1.2e+04
      -4000/2 | 1000 x 320  G=32 |    5.9e-04 |     1.4e-04 | 2.4e-03 | 3.4e+00
      -4000/2 | 4096 x 128  G=32 |    5.4e-04 |     1.8e-04 | 2.2e-03 | 3.4e+00
      -4000/2 | 64 x 2560 G=32   |    5.7e-04 |     2.0e-04 | 2.3e-03 | 1.4e+01
      -4000/2 | 256 x 960  G=32  |    8.4e-04 |     1.6e-04 | 3.4e-03 | 6.8e+00
      -4000/2 | 300 x 64   G=1   |    6.3e-04 |     1.7e-04 | 2.5e-03 | 7.8e+00
      0/0.001 | 64 x 320  G=32   |    8.9e-07 |     8.3e-07 | 2.0e-05 | 8.3e-07
      0/0.001 | 1000 x 320  G=32 |    7.8e-07 |     1.1e-06 | 2.0e-05 | 9.4e-07
      0/0.001 | 4096 x 128  G=32 |    9.7e-07 |     1.1e-06 | 2.0e-05 | 9.7e-07
      0/0.001 | 64 x 2560 G=32   |    8.3e-07 |     1.0e-06 | 2.0e-05 | 1.0e-06
      0/0.001 | 256 x 960  G=32  |    9.6e-07 |     1.0e-06 | 2.0e-05 | 9.6e-07
      0/0.001 | 300 x 64   G=1   |    7.0e-07 |     8.7e-07 | 2.0e-05 | 1.3e-06
   1000/0.001 | 64 x 320  G=32   |    1.2e-01 |     5.3e-02 | 4.8e-01 | 5.2e+00
   1000/0.001 | 1000 x 320  G=32 |    9.9e-02 |     4.3e-02 | 4.0e-01 | 6.5e+00
   1000/0.001 | 4096 x 128  G=32 |    1.5e-01 |     4.2e-02 | 6.1e-01 | 9.8e+00
   1000/0.001 | 64 x 2560 G=32   |    1.7e-01 |     6.3e-02 | 6.8e-01 | 7.4e+00
   1000/0.001 | 256 x 960  G=32  |    1.8e-01 |     3.8e-02 | 7.3e-01 | 7.6e+00
   1000/0.001 | 300 x 64   G=1   |    1.5e-01 |     1.3e-02 | 6.1e-01 | 8.3e+00
    per-group | 64 x 320  G=32   |    3.3e-04 |     7.3e-05 | 1.3e-03 | 1.1e+00
    per-group | 1000 x 320  G=32 |    2.6e-04 |     1.2e-04 | 1.0e-03 | 6.9e-01
    per-group | 4096 x 128  G=32 |    1.4e-04 |     7.3e-05 | 5.7e-04 | 4.9e-01
    per-group | 64 x 2560 G=32   |    2.4e-04 |     8.3e-05 | 9.6e-04 | 6.4e-01
    per-group | 256 x 960  G=32  |    1.9e-04 |     8.6e-05 | 7.8e-04 | 5.5e-01
    per-group | 300 x 64   G=1   |    8.7e-07 |     1.2e-06 | 2.0e-05 | 3.5e-06
   per-sample | 64 x 320  G=32   |    2.2e-04 |     8.1e-05 | 8.9e-04 | 2.4e+00
   per-sample | 1000 x 320  G=32 |    2.6e-04 |     7.5e-05 | 1.0e-03 | 7.7e-01
   per-sample | 4096 x 128  G=32 |    2.0e-04 |     5.2e-05 | 8.1e-04 | 6.9e-01
   per-sample | 64 x 2560 G=32   |    2.4e-04 |     1.2e-04 | 9.6e-04 | 1.7e+00
   per-sample | 256 x 960  G=32  |    1.8e-04 |     8.6e-05 | 7.3e-04 | 7.7e-01
   per-sample | 300 x 64   G=1   |    1.0e-04 |     1.3e-05 | 4.0e-04 | 4.1e+00
outlier-pixel | 64 x 320  G=32   |    4.0e-06 |     2.4e-06 | 2.0e-05 | 4.1e-04
outlier-pixel | 1000 x 320  G=32 |    2.0e-05 |     1.1e-05 | 7.8e-05 | 8.4e-03
outlier-pixel | 4096 x 128  G=32 |    2.0e-05 |     1.6e-05 | 8.1e-05 | 5.7e-02
outlier-pixel | 64 x 2560 G=32   |    6.2e-06 |     3.4e-06 | 2.5e-05 | 2.0e-04
outlier-pixel | 256 x 960  G=32  |    9.4e-06 |     5.3e-06 | 3.7e-05 | 1.1e-03
outlier-pixel | 300 x 64   G=1   |    4.7e-06 |     4.1e-06 | 2.0e-05 | 1.7e-02
     constant | 64 x 320  G=32   |    1.1e-01 |     1.3e-07 | 4.3e-01 | 1.2e-01
     constant | 1000 x 320  G=32 |    1.1e-01 |     1.3e-07 | 4.3e-01 | 1.2e-01
     constant | 4096 x 128  G=32 |    1.1e-01 |     8.3e-08 | 4.3e-01 | 1.2e-01
     constant | 64 x 2560 G=32   |    1.1e-01 |     2.5e-07 | 4.3e-01 | 1.2e-04
     constant | 256 x 960  G=32  |    1.1e-01 |     2.1e-07 | 4.3e-01 | 1.2e-01
     constant | 300 x 64   G=1   |    5.7e-02 |     8.3e-08 | 2.3e-01 | 4.3e+00
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from oracle import mx8

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
# tests/test_kernels_gpu.py's TOL and close(), copied: the 16-bit tolerance of every norm test in the suite
TOL = {F16: dict(rtol=2e-3, atol=2e-3), BF16: dict(rtol=1.6e-2, atol=1.6e-2)}


def close(out, ref, dtype, scale=1.0, msg=""):
    t = TOL[dtype]
    torch.testing.assert_close(out.float().cpu(), ref.float(), rtol=t["rtol"], atol=t["atol"] * scale, msg=lambda m: f"{msg}: {m}")


def randn64(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ------------------------------------------------------------------ input families
# (offset, std) per storage type: the spacing of the type at `offset` is <= std / 4, so the rounded data keeps roughly that std
OFFSETS = {
    F32: [(0.5, 2.0), (16.0, 1.0), (64.0, 1.0), (256.0, 1.0), (1000.0, 1.0), (100.0, 0.1), (4000.0, 2.0),
          (-16.0, 1.0), (-64.0, 1.0), (-256.0, 1.0), (-1000.0, 1.0), (-100.0, 0.1), (-4000.0, 2.0), (0.0, 1e-3), (1000.0, 1e-3)],
    F16: [(0.5, 2.0), (16.0, 1.0), (64.0, 1.0), (256.0, 1.0), (-256.0, 1.0), (0.0, 1e-3), (3e4, 1e3)],
    BF16: [(0.5, 2.0), (8.0, 1.0), (32.0, 1.0), (0.0, 1e-3)],
}
BIG = {F32: 1000.0, F16: 256.0, BF16: 32.0}              # the large offset (std 1) of the structured families
GROUP_STEP = {F32: 300.0, F16: 80.0, BF16: 8.0}          # group g sits at (g % 4) * step
CONSTANT = {F32: 1000.125, F16: 100.0, BF16: 100.0}      # exactly representable
FAMILIES = {dt: [f"{o:g}/{s:g}" for o, s in OFFSETS[dt]] + ["per-group", "per-sample", "outlier-pixel", "constant"] for dt in OFFSETS}


def family(name, dtype, B, HW, C, groups, seed=0):
    """float64 (B, HW, C), not yet rounded to the storage type"""
    z = randn64(B, HW, C, seed=seed)
    if name == "per-group":          # a pivot shared by several groups must not pass by accident
        g = torch.arange(C) // (C // groups)
        return z + ((g % 4).double() * GROUP_STEP[dtype])[None, None, :]
    if name == "per-sample":         # ... nor one shared by the samples of a batch
        return z + (torch.arange(B).double() * BIG[dtype] / max(B - 1, 1))[:, None, None]
    if name == "outlier-pixel":      # ... nor one taken from the first element
        x = z + BIG[dtype]
        x[:, 0, :] = 0.0
        return x
    if name == "constant":
        return torch.full((B, HW, C), CONSTANT[dtype], dtype=torch.float64)
    o, s = (float(t) for t in name.split("/"))
    return z * s + o


# HW, C1, C2, groups: every path of gn_run
def _id(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else "x".join(map(str, v)) if isinstance(v, tuple) else None


GN_SHAPES = [
    (64, 320, 0, 32),         # one chunk (HW * C <= 32768)
    (1000, 320, 0, 32),       # ten chunks, a ragged last one
    (4096, 128, 0, 32),       # sixteen chunks of four channels per group
    (64, 1280, 1280, 32),     # two vectors per lane (C > 2048), fused concat
    (256, 640, 320, 32),      # fused concat, the halves at different offsets; group 21 straddles them
    (300, 64, 0, 1),          # one group
]


def gn_case(dtype, fam, HW, C1, C2, groups, B=2):
    C = C1 + C2
    x = family(fam, dtype, B, HW, C, groups, seed=HW + C)
    o = float(fam.split("/")[0]) if "/" in fam else BIG[dtype]
    if C2 and fam != "constant" and o != 0.0:        # the second half of the concat sits somewhere else (not the tiny-spread family:
        x[:, :, C1:] += -0.5 * o + 3.0               # 16-bit storage could not hold its std away from zero)
    x = x.to(dtype)
    gamma = randn64(C, seed=1).to(dtype)
    beta = randn64(C, seed=2).to(dtype)
    return x, gamma, beta


def gn_ref(x, gamma, beta, groups, eps, silu, fam):
    """float64 F.group_norm of the stored values (NHWC <-> NCHW as in test_groupnorm); a constant tensor gives exactly beta"""
    if fam == "constant":
        ref = beta.double()[None, None, :].expand(x.shape).clone()
    else:
        ref = F.group_norm(x.double().transpose(1, 2), groups, gamma.double(), beta.double(), eps).transpose(1, 2)
    return F.silu(ref) if silu else ref


def gn_run(x, gamma, beta, groups, eps, silu, C1, C2, dev):
    xd = x.to(dev)
    x1 = xd[:, :, :C1].contiguous()
    x2 = xd[:, :, C1:].contiguous() if C2 else None
    return ops.groupnorm(x1, gamma.to(dev), beta.to(dev), groups, eps, silu=silu, x2=x2)


# ------------------------------------------------------------------ 1. GroupNorm
@pytest.mark.parametrize("shape", GN_SHAPES, ids=_id)
@pytest.mark.parametrize("dtype,fam", [(dt, f) for dt in (F16, BF16) for f in FAMILIES[dt]], ids=_id)
def test_groupnorm_conditioning_16bit(dev, dtype, fam, shape):
    HW, C1, C2, groups = shape
    x, gamma, beta = gn_case(dtype, fam, HW, C1, C2, groups)
    for silu in (False, True):
        y = gn_run(x, gamma, beta, groups, 1e-5, silu, C1, C2, dev)
        close(y, gn_ref(x, gamma, beta, groups, 1e-5, silu, fam), dtype, scale=2.0, msg=f"{fam} silu={silu}")


@pytest.mark.parametrize("shape", GN_SHAPES, ids=_id)
@pytest.mark.parametrize("fam", FAMILIES[F32])
def test_groupnorm_conditioning_fp32(dev, shape, fam):
    """fp32 storage (the up blocks of the upcast VAE decode).  The bound comes from torch's own fp32 error on the same input."""
    HW, C1, C2, groups = shape
    eps = 1e-6
    x, gamma, beta = gn_case(F32, fam, HW, C1, C2, groups)
    worst = []
    for silu in (False, True):
        ref = gn_ref(x, gamma, beta, groups, eps, silu, fam)
        t32 = F.group_norm(x.transpose(1, 2), groups, gamma, beta, eps).transpose(1, 2)
        yard = ((F.silu(t32) if silu else t32).double() - ref).abs().max().item()
        limit = max(2e-5, 4.0 * yard)
        y = gn_run(x, gamma, beta, groups, eps, silu, C1, C2, dev)
        err = (y.double().cpu() - ref).abs().max().item()
        worst.append((err / limit, yard, err, limit))
    _, yard, err, limit = max(worst)
    print(f"\nFP32GN | {fam:>13} | {HW:>4} x {C1 + C2:<4} G={groups:<2} | torch-fp32 {yard:.1e} | kernel {err:.1e} | limit {limit:.1e}")
    for ratio, yard, err, limit in worst:
        assert err <= limit, f"{fam} {shape}: kernel max|d| {err:.3e} > limit {limit:.3e} (torch fp32: {yard:.3e})"


@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=_id)
def test_groupnorm_offset_input_is_bitwise_deterministic(dev, dtype):
    HW, C1, C2, groups = 1000, 320, 0, 32
    x, gamma, beta = gn_case(dtype, f"{BIG[dtype]:g}/1", HW, C1, C2, groups)
    a = gn_run(x, gamma, beta, groups, 1e-5, True, C1, C2, dev)
    b = gn_run(x, gamma, beta, groups, 1e-5, True, C1, C2, dev)
    assert torch.equal(a, b), "GroupNorm must be bitwise deterministic"
    x, gamma, beta = gn_case(dtype, "per-group", 64, 1280, 1280, 32)
    a = gn_run(x, gamma, beta, 32, 1e-5, False, 1280, 1280, dev)
    b = gn_run(x, gamma, beta, 32, 1e-5, False, 1280, 1280, dev)
    assert torch.equal(a, b), "GroupNorm must be bitwise deterministic"


# ------------------------------------------------------------------ 2. GroupNorm -> MX-fp8
@pytest.mark.parametrize("dtype,fam", [(F16, "256/1"), (BF16, "32/1")])
@pytest.mark.parametrize("B,H,W,C", [(2, 9, 9, 320), (2, 16, 16, 640)])
def test_groupnorm_mx8_is_the_quantised_groupnorm_on_offset_input(dev, dtype, fam, B, H, W, C):
    """tests/test_mx8_gpu.py::test_groupnorm_mx8_is_the_quantised_groupnorm's assertion where mean >> std: both instantiations of
    gn_apply_kernel must see the same statistics and run the same arithmetic."""
    x, gamma, beta = gn_case(dtype, fam, H * W, C, 0, 32, B=B)
    x1, gamma, beta = x.reshape(B, H, W, C).to(dev), gamma.to(dev), beta.to(dev)
    y = ops.groupnorm(x1, gamma, beta, 32, 1e-5, silu=True)
    got = ops.groupnorm_mx8(x1, gamma, beta, 32, 1e-5, silu=True)
    Cq = (C + 127) // 128 * 128
    yp = torch.zeros(B * H * W, Cq)
    yp[:, :C] = y.float().cpu().reshape(-1, C)
    q, packed, _ = mx8.quantize(yp)
    assert got.q.shape == (B, H, W, Cq) and got.scales.shape == (Cq // 128, B * H * W)
    assert torch.equal(got.q.cpu().reshape(-1, Cq), q), f"{(got.q.cpu().reshape(-1, Cq) != q).sum().item()} element bytes differ"
    assert torch.equal(got.scales.cpu(), packed)
    close(y.reshape(B, H * W, C), gn_ref(x, gamma.cpu(), beta.cpu(), 32, 1e-5, True, fam), dtype, scale=2.0, msg=fam)


# ------------------------------------------------------------------ 3. LayerNorm
LN_FAMILIES = {F16: [f"{o:g}/{s:g}" for o, s in OFFSETS[F16]] + ["constant"], BF16: [f"{o:g}/{s:g}" for o, s in OFFSETS[BF16]] + ["constant"]}


def ln_ref(x, gamma, beta, eps):
    return F.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("C", [8, 64, 520, 640, 1280, 2048])
@pytest.mark.parametrize("M", [1, 5, 77, 300])
def test_layernorm_conditioning(dev, dtype, M, C):
    """The kernel's two-pass variance, pinned: every family of the type at this shape."""
    gamma, beta = randn64(C, seed=1).to(dtype), randn64(C, seed=2).to(dtype)
    for k, fam in enumerate(LN_FAMILIES[dtype]):
        x = family(fam, dtype, 1, M, C, 1, seed=M + C + k)[0].to(dtype)
        y = ops.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), 1e-5)
        ref = beta.double()[None, :].expand(M, C) if fam == "constant" else ln_ref(x, gamma, beta, 1e-5)
        close(y, ref, dtype, scale=2.0, msg=fam)


@pytest.mark.parametrize("dtype,step", [(F16, 50.0), (BF16, 8.0)])
@pytest.mark.parametrize("M,C", [(77, 640), (300, 520), (5, 2048), (1, 64)])
def test_layernorm_strided_rows_with_per_row_offsets(dev, dtype, step, M, C):
    """x is a column slice of a wider buffer (ldx = C + 64 > C, 16-byte aligned); row r sits at (r % 5) * step."""
    big = randn64(M, C + 64, seed=M + C) + ((torch.arange(M) % 5).double() * step)[:, None]
    big = big.to(dtype)
    gamma, beta = randn64(C, seed=1).to(dtype), randn64(C, seed=2).to(dtype)
    bd = big.to(dev)
    xs = bd[:, 32:32 + C]
    assert xs.stride(0) == C + 64 and xs.data_ptr() % 16 == 0
    y = ops.layernorm(xs, gamma.to(dev), beta.to(dev), 1e-5)
    close(y, ln_ref(big[:, 32:32 + C], gamma, beta, 1e-5), dtype, scale=2.0)
    assert torch.equal(bd.cpu(), big), "the input buffer must not change"


@pytest.mark.parametrize("dtype,fam", [(F16, "256/1"), (BF16, "32/1")])
@pytest.mark.parametrize("M,C", [(77, 640), (300, 1280)])
def test_layernorm_mx8_equals_layernorm_then_quantise_on_offset_input(dev, dtype, fam, M, C):
    x = family(fam, dtype, 1, M, C, 1, seed=3)[0].to(dtype).to(dev)
    g, b = (randn64(C, seed=1) + 1).to(dtype).to(dev), randn64(C, seed=2).to(dtype).to(dev)
    fused = ops.layernorm_mx8(x, g, b, 1e-5)
    y = ops.layernorm(x, g, b, 1e-5)
    two = ops.quant_mx8(y)
    assert torch.equal(fused.q, two.q) and torch.equal(fused.scales[:, :M], two.scales[:, :M])
    q, packed, _ = mx8.quantize(y.float().cpu())
    assert torch.equal(fused.q.cpu(), q) and torch.equal(fused.scales.cpu()[:, :M], packed)


def test_layernorm_rejects_what_it_cannot_run(dev):
    """Argument validation only: the call returns an error before anything is launched."""
    g, b = torch.ones(2056, dtype=F16, device=dev), torch.zeros(2056, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError):
        ops.layernorm(torch.zeros(4, 2056, dtype=F16, device=dev), g, b, 1e-5)              # C > 2048
    wide = torch.zeros(4, 64 + 60, dtype=F16, device=dev)
    xs = wide[:, 32:32 + 64]
    assert xs.stride(0) % 8 != 0
    with pytest.raises(L.OmgHipError):
        ops.layernorm(xs, g[:64], b[:64], 1e-5)                                             # ldx % 8 != 0


# ------------------------------------------------------------------ 4. softmax_rows_
SM_TOL = {F16: dict(rtol=4e-3, atol=1e-5), BF16: dict(rtol=2e-2, atol=1e-5)}      # tests/test_vae_gpu.py::test_softmax_rows_and_channel_mix


def softmax_check(dev, x, scale, dtype, pad=24):
    """x: (rows, cols) already in `dtype`; runs in a wider buffer and checks values and the untouched padding"""
    rows, cols = x.shape
    big = torch.full((rows, cols + pad), 7.0, dtype=dtype)
    big[:, :cols] = x
    bd = big.to(dev)
    ops.softmax_rows_(bd[:, :cols], scale)
    out = bd.cpu()
    assert torch.equal(out[:, cols:].view(torch.int16), big[:, cols:].view(torch.int16)), "padding columns were written"
    ref = torch.softmax(x.double() * scale, dim=-1)
    torch.testing.assert_close(out[:, :cols].double(), ref, **SM_TOL[dtype])
    return out[:, :cols], ref


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
def test_softmax_text_encoder_causal_mask(dev, dtype):
    """An 80 x 80 score block plus the additive causal mask of omg_amd/text_encoder.py (-30000 above the diagonal), scale 1."""
    T = 80
    mask = torch.zeros(T, T, dtype=dtype).masked_fill_(torch.ones(T, T, dtype=torch.bool).triu(1), -30000.0)
    scores = (randn64(T, T, seed=0) * 3).to(dtype)
    x = (scores.float() + mask.float()).to(dtype)
    out, ref = softmax_check(dev, x, 1.0, dtype)
    dead = torch.ones(T, T, dtype=torch.bool).triu(1)
    assert bool((out[dead] == 0).all()), "masked columns must be exactly zero"
    assert out[0, 0].item() == 1.0                                    # row 0: one live column
    rt = SM_TOL[dtype]["rtol"]
    assert bool(((out.double().sum(-1) - 1).abs() <= rt).all())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
def test_softmax_edge_rows(dev, dtype):
    cols = 300
    z = randn64(8, cols, seed=1)
    x = z.clone()
    x[0] = 0.0                              # all equal
    x[1] = -7.25                            # all equal, not zero
    x[2] = 65504.0                          # all equal at the top of fp16
    x[3, 17], x[3, 200] = 65504.0, -65504.0
    x[4, 0], x[4, cols - 1] = -65504.0, 65504.0
    x[5, 100] += 60.0                       # one entry 60 above the rest
    x[6, 5], x[6, 6] = 65504.0, 65504.0     # a tie at the top
    x = x.to(dtype)
    for scale in (1.0, 0.125):
        out, ref = softmax_check(dev, x, scale, dtype)
        assert bool((out[:3] == out[:3, :1]).all()), "constant rows must come out constant"
        assert out[3, 17].item() == 1.0 and out[4, cols - 1].item() == 1.0 and out[3, 200].item() == 0.0
        assert out[6, 5].item() == 0.5 and out[6, 6].item() == 0.5


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("rows", [1, 70])
@pytest.mark.parametrize("cols", [1, 77, 255, 256, 257, 1000, 16384])
def test_softmax_shapes_and_padding(dev, dtype, rows, cols):
    x = (randn64(rows, cols, seed=rows + cols) * 3).to(dtype)
    softmax_check(dev, x, 0.37, dtype)


# ------------------------------------------------------------------ 5. entry points without a direct test
@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("n", [8, 8 * 256 * 4096 + 8 * 37, 80 * 80])
def test_add_inplace_is_the_rounded_fp32_sum(dev, dtype, n):
    """8 * 256 * 4096 + 8 * 37: one pass of the capped grid plus a ragged second trip of the grid-stride loop; 80 * 80: the mask add."""
    g = torch.Generator().manual_seed(n % 1000)
    y, a = (torch.randn(n, generator=g) * 3).to(dtype), torch.randn(n, generator=g).to(dtype)
    yd, ad = y.to(dev), a.to(dev)
    r = ops.add_(yd, ad)
    assert r.data_ptr() == yd.data_ptr()
    want = (y.float() + a.float()).to(dtype)
    assert torch.equal(yd.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(ad.cpu().view(torch.int16), a.view(torch.int16)), "the addend must not change"


def test_add_inplace_rejects_a_ragged_length(dev):
    y = torch.zeros(12, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError):
        ops.add_(y, torch.ones(12, dtype=F16, device=dev))
    assert bool((y == 0).all())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=_id)
@pytest.mark.parametrize("n", [8, 1000, 256 * 1024 + 3])
def test_gather_step_reads_the_device_counter(dev, dtype, n):
    S = 5
    table = torch.randn(S, n, generator=torch.Generator().manual_seed(n)).to(dtype)
    td = table.to(dev)
    for s in (0, 2, S - 1):
        idx = torch.tensor([s], dtype=torch.int32, device=dev)
        out = torch.full((n,), -1.0, dtype=dtype, device=dev)
        ops.gather_step(td, idx, out)
        assert torch.equal(out.cpu().view(torch.int16), table[s].view(torch.int16))
        assert idx.item() == s
    assert torch.equal(td.cpu().view(torch.int16), table.view(torch.int16))


@pytest.mark.parametrize("out_dtype", [F16, BF16, F32], ids=_id)
@pytest.mark.parametrize("H,W", [(24, 20), (128, 128)])
def test_scale_model_input_bitwise(dev, out_dtype, H, W):
    lat = torch.randn(2, 4, H, W, generator=torch.Generator().manual_seed(H)) * 13.0
    cin = torch.tensor([1.0 / math.sqrt(14.6146 ** 2 + 1.0)], dtype=torch.float32)
    out = torch.full((4, 4, H, W), -1.0, dtype=out_dtype, device=dev)
    ld = lat.to(dev)
    ops.scale_model_input(ld, cin.to(dev), out)
    want = (torch.cat([lat, lat]) * cin).to(out_dtype)
    assert torch.equal(out.cpu(), want) and torch.equal(ld.cpu(), lat)


def _grid(n, gen):
    """randn rounded to multiples of 2^-10: sums of two or three such values are exact in fp32, so the fused noise is"""
    return (torch.randn(*n, generator=gen) * 1024).round() / 1024


@pytest.mark.parametrize("out_dtype", [None, F16, BF16, F32])
@pytest.mark.parametrize("advance", [True, False])
@pytest.mark.parametrize("fuse", [True, False])
def test_fuse_cfg_step_against_a_float64_restatement(dev, fuse, advance, out_dtype):
    """The plain step kernel against include/omg_hip.h's contract, restated in float64:
        nearest mask resize  src = floor(dst * in / out)
        new  = edit * [union == 0] + sum_c region_c * [mask_c == 1]        (edited sample only; overlaps sum)
        eps  = unc + gs * (cnd - unc);   latents' = cx * latents + ce * eps;   model_input' = cin_next * latents'
    Four concepts: two overlapping masks, one concept without a mask, one mask without a region prediction (its pixels drop the
    edit and add nothing).  Mask values 0.5 and 2.0 are not 1.0: off.  Masks 200 x 168 over a 24 x 20 latent: not a multiple.

    Tolerance of the fp32 latents.  The kernel runs, with u = 2^-24 and every operation rounded once,
        d = cnd - unc;  e = fma(gs, d, unc);  t = cx * x;  l = fma(ce, e, t).
    |d - d*| <= u |d*|;  |e - e*| <= gs u |d*| + u (gs |d*| + |unc|) (1 + u);  |t - t*| <= u |cx x|;
    |l - l*| <= |ce| |e - e*| + u |cx x| + u (|ce e*| + |cx x|) (1 + ..) <= u (2 |cx x| + |ce| (2 |unc| + 3 gs |d*|)) + O(u^2)
             <= 3 u Bd  <  4 u Bd,   Bd = |cx x| + |ce| (|unc| + gs |cnd - unc|).
    unc / cnd are the FUSED values; the inputs lie on a 2^-10 grid so that the overlap sums are exact in fp32 and the fusion adds
    no rounding of its own (fused_noise_out is compared for equality).  model_input' in fp32 is one more multiply:
    |cin| 3 u Bd + u |cin l*| <= 4 u |cin| Bd.  16-bit model inputs are the kernel's own fp32 latents times cin, rounded: one ulp."""
    C, H, W, Hm, Wm, gs, S, s0 = 4, 24, 20, 200, 168, 7.5, 6, 3
    gen = torch.Generator().manual_seed(5)
    noise, lat = _grid((4, C, H, W), gen), torch.randn(2, C, H, W, generator=gen) * 5
    regions = [_grid((2, C, H, W), gen), _grid((2, C, H, W), gen), _grid((2, C, H, W), gen), None]
    yy, xx = torch.arange(Hm)[:, None], torch.arange(Wm)[None, :]
    mA = ((yy >= 20) & (yy < 120) & (xx >= 10) & (xx < 100)).float()
    mB = ((yy >= 70) & (yy < 180) & (xx >= 60) & (xx < 160)).float()        # overlaps mA
    mA[30:50, 20:40] = 0.5                                                   # not exactly 1: off
    mB[150:170, 100:150] = 2.0
    mD = ((yy >= 130) & (xx < 50)).float()                                   # a mask without a region prediction
    mD[190:, :] = 0.5
    masks = [mA, mB, None, mD]
    coef = torch.rand(S, 4, generator=gen) * torch.tensor([0.2, -0.3, 1.0, 0.0]) + torch.tensor([1.0, -0.05, 0.05, 0.0])
    cx, ce, cin = (coef[s0, k].double() for k in range(3))

    # float64 restatement
    n64, l64 = noise.double(), lat.double()
    unc, cnd = n64[:2].clone(), n64[2:].clone()
    if fuse:
        my, mx = (torch.arange(H) * Hm) // H, (torch.arange(W) * Wm) // W
        union = torch.zeros(H, W, dtype=torch.bool)
        add = torch.zeros(2, C, H, W, dtype=torch.float64)
        for r, m in zip(regions, masks):
            if m is None:
                continue
            on = m[my][:, mx] == 1.0
            union |= on
            if r is not None:
                add += r.double() * on
        unc[1] = torch.where(union, 0.0, unc[1]) + add[0]
        cnd[1] = torch.where(union, 0.0, cnd[1]) + add[1]
        assert union.any() and not union.all()
    eps = unc + gs * (cnd - unc)
    lref = cx * l64 + ce * eps
    bound = 4 * 2.0 ** -24 * ((cx * l64).abs() + ce.abs() * (unc.abs() + gs * (cnd - unc).abs()))

    d = lambda t: None if t is None else t.to(dev)
    lat_d, idx = lat.to(dev), torch.tensor([s0], dtype=torch.int32, device=dev)
    mi = None if out_dtype is None else torch.full((4, C, H, W), -1.0, dtype=out_dtype, device=dev)
    tap = torch.full((2, C, H, W), -1.0, device=dev) if fuse else None
    ops.fuse_cfg_step(noise.to(dev), lat_d, coef.to(dev), idx, guidance_scale=gs, fuse=fuse, region_preds=[d(r) for r in regions],
                      masks=[d(m) for m in masks], model_input_next=mi, advance=advance, fused_noise_out=tap)
    assert idx.item() == s0 + int(advance)
    got = lat_d.cpu()
    err = (got.double() - lref).abs()
    assert bool((err <= bound).all()), f"latents: worst {(err / bound).max().item():.2f} x the bound"
    if fuse:
        assert torch.equal(tap.cpu().double(), torch.stack([unc[1], cnd[1]])), "fused noise"
    if out_dtype == F32:
        e2 = (mi.cpu().double() - cin * torch.cat([lref, lref])).abs()
        b2 = cin.abs() * torch.cat([bound, bound]) * (1 + 2.0 ** -20)
        assert bool((e2 <= b2).all()), f"model input: worst {(e2 / b2).max().item():.2f} x the bound"
    elif out_dtype is not None:
        want = (torch.cat([got, got]) * coef[s0, 2]).to(out_dtype).double()
        ulp = 2.0 ** (-10 if out_dtype == F16 else -7)
        assert bool(((mi.cpu().double() - want).abs() <= ulp * want.abs()).all())
        assert torch.equal(mi[:2], mi[2:])
