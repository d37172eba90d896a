"""Thin torch-tensor wrappers over the C ABI (``include/omg_hip.h``).

PyTorch here is plumbing only: it owns device memory (``torch.empty``), the current
HIP stream and nothing else — every arithmetic op below is a hand-written gfx950
kernel in ``omg_amd/csrc``.  All wrappers launch on ``torch.cuda.current_stream()``
so they are captured by ``torch.cuda.graph`` (hipGraph) like any torch op.
Tensors must live on a ROCm device; a CPU tensor raises (no fallback).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L

_DT = {torch.float16: L.OMG_F16, torch.bfloat16: L.OMG_BF16}


def _dt(t: torch.Tensor, allow_f32: bool = False) -> int:
    if allow_f32 and t.dtype == torch.float32:
        return L.OMG_F32
    try:
        return _DT[t.dtype]
    except KeyError:
        raise L.OmgHipError(f"unsupported dtype {t.dtype}; use float16 or bfloat16") from None


def _dev(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise L.OmgHipError("omg_amd ops need tensors on the MI355X (cuda/hip device); there is no CPU fallback")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class KernelProfiler:
    """Opt-in per-launch timing with HIP events on the launch stream (used by bench.py's roofline leg).
    Off by default: the product path records nothing."""

    def __init__(self):
        self.records = []   # (kind, flops, start_event, end_event)

    def begin(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream())
        return e

    def end(self, kind: str, flops: float, start, tag=None) -> None:
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream())
        self.records.append((kind, flops, start, e, tag))

    def summary(self):
        """kind -> dict(launches, ms, flops); call after torch.cuda.synchronize()."""
        out = {}
        for kind, fl, s, e, _ in self.records:
            d = out.setdefault(kind, dict(launches=0, ms=0.0, flops=0.0))
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += fl
        return out

    def by_tag(self):
        """(kind, tag) -> dict(launches, ms, flops), sorted by total time."""
        out = {}
        for kind, fl, s, e, tag in self.records:
            d = out.setdefault((kind, tag), dict(launches=0, ms=0.0, flops=0.0))
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += fl
        return sorted(out.items(), key=lambda kv: -kv[1]["ms"])


_PROF: Optional[KernelProfiler] = None


def set_profiler(p: Optional[KernelProfiler]) -> None:
    global _PROF
    _PROF = p


class LoraSpec:
    """Second K-segment of a GEMM: ``C += A2 @ W2[adapter]^T`` (PEFT ``s * B(A(x))``)."""

    __slots__ = ("a2", "w2", "group_adapter", "a2_col_block")

    def __init__(self, a2: torch.Tensor, w2: torch.Tensor, group_adapter: Optional[torch.Tensor] = None,
                 a2_col_block: int = 0):
        self.a2, self.w2, self.group_adapter, self.a2_col_block = a2, w2, group_adapter, a2_col_block


def gemm(a: torch.Tensor, w: torch.Tensor, *, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, act: int = L.ACT_NONE, out: Optional[torch.Tensor] = None,
         out_scale: float = 1.0, group_bias: Optional[torch.Tensor] = None, groups: int = 1,
         lora: Optional[LoraSpec] = None, w_group_adapter: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[M, N_out] = epi(a[M,K] @ w[N,K]^T)``; see ``omg_gemm`` in include/omg_hip.h.

    ``w`` may be 3-D ``[n_adapters, N, K]`` together with ``w_group_adapter`` (int32 device
    tensor, one adapter id per group) — the LoRA-down projection of a batch whose samples
    use different adapters.
    """
    _dev(a)
    M, K = a.shape
    assert a.stride(1) == 1
    if w.dim() == 3:
        N = w.shape[1]
        w_stride = w.stride(0)
        ldw = w.stride(1)
    else:
        N = w.shape[0]
        w_stride = 0
        ldw = w.stride(0)
    assert w.shape[-1] == K and w.stride(-1) == 1
    n_out = N // 2 if act == L.ACT_GEGLU else N
    if out is None:
        out = torch.empty((M, n_out), dtype=a.dtype, device=a.device)
    assert out.stride(1) == 1 and out.shape[0] == M and out.shape[1] == n_out
    args = L.GemmArgs()
    args.dtype = _dt(a)
    args.M, args.N, args.K = M, N, K
    args.A, args.lda = a.data_ptr(), a.stride(0)
    args.W, args.ldw = w.data_ptr(), ldw
    args.groups = groups
    args.rows_per_group = M // groups
    adapter = w_group_adapter
    if lora is not None:
        a2, w2 = lora.a2, lora.w2
        args.A2, args.lda2 = a2.data_ptr(), a2.stride(0)
        args.K2 = w2.shape[-1]
        args.W2 = w2.data_ptr()
        if w2.dim() == 3:
            args.ldw2, args.w2_adapter_stride = w2.stride(1), w2.stride(0)
        else:
            args.ldw2, args.w2_adapter_stride = w2.stride(0), 0
        args.a2_col_block = lora.a2_col_block
        if lora.group_adapter is not None:
            adapter = lora.group_adapter
    args.group_adapter = _p(adapter)
    args.w_adapter_stride = w_stride
    args.bias = _p(bias)
    if group_bias is not None:
        args.group_bias, args.ldgb = group_bias.data_ptr(), group_bias.stride(0)
    if residual is not None:
        assert residual.stride(1) == 1
        args.residual, args.ldr = residual.data_ptr(), residual.stride(0)
    args.act = act
    args.out_scale = out_scale
    args.C, args.ldc = out.data_ptr(), out.stride(0)
    if _PROF is not None:
        t0 = _PROF.begin()
        L.check(L.lib().omg_gemm(C.byref(args), _stream()), "omg_gemm")
        _PROF.end("gemm", 2.0 * M * N * (K + args.K2), t0, ("lin", M, N, K, args.K2, groups if adapter is not None else 1, act))
        return out
    L.check(L.lib().omg_gemm(C.byref(args), _stream()), "omg_gemm")
    return out


class Mx8Tensor:
    """An MX-fp8 quantised 2-D operand: ``q`` uint8 [rows, K] (OCP e4m3), ``scales`` int32 [K/128, s_ld] (four E8M0 bytes per
    (row, 128-wide stage), stage-major — the layout omg_gemm_mx8 stages with one LDS-DMA per tile and stage)."""

    __slots__ = ("q", "scales", "rows", "K", "shape")

    def __init__(self, q: torch.Tensor, scales: torch.Tensor, shape=None):
        self.q, self.scales, self.rows, self.K = q, scales, q.shape[0], q.shape[1]
        self.shape = tuple(shape) if shape is not None else (q.shape[0], q.shape[1])      # logical shape (..., K) of the activation

    @property
    def device(self):
        return self.q.device


def quant_mx8(x: torch.Tensor, out: Optional[Mx8Tensor] = None) -> Mx8Tensor:
    """fp16 / bf16 [..., K] (rows with one common stride, unit inner stride) -> :class:`Mx8Tensor` (omg_quant_mx8)."""
    _dev(x)
    shape = x.shape
    x = x.reshape(-1, shape[-1])
    assert x.stride(1) == 1
    M, K = x.shape
    if K % 128 != 0:
        raise L.OmgHipError("MX-fp8 operands need K % 128 == 0")
    if out is None:
        s_ld = (M + 3) // 4 * 4
        out = Mx8Tensor(torch.empty((M, K), dtype=torch.uint8, device=x.device),
                        torch.zeros((K // 128, s_ld), dtype=torch.int32, device=x.device), shape)
    assert out.q.shape == (M, K) and out.q.stride(1) == 1 and out.scales.shape[0] == K // 128
    L.check(L.lib().omg_quant_mx8(_dt(x), x.data_ptr(), x.stride(0), M, K, out.q.data_ptr(), out.q.stride(0),
                                  out.scales.data_ptr(), out.scales.stride(0), _stream()), "omg_quant_mx8")
    return out


def gemm_mx8(a: Mx8Tensor, w: Mx8Tensor, *, out_dtype: torch.dtype = torch.float16, bias: Optional[torch.Tensor] = None,
             residual: Optional[torch.Tensor] = None, act: int = L.ACT_NONE, out: Optional[torch.Tensor] = None,
             out_scale: float = 1.0, groups: int = 1, w_group_adapter: Optional[torch.Tensor] = None,
             n_per_adapter: Optional[int] = None, out_mx8: bool = False):
    """``out[M, N_out] = epi(dequant(a) @ dequant(w)^T)`` on the block-scaled fp8 MFMA (omg_gemm_mx8).

    ``out_mx8`` (GEGLU only, N % 256 == 0): return the result as an :class:`Mx8Tensor` — the next MX-fp8 Linear's operand,
    quantised in the epilogue, bit-identical to ``quant_mx8`` of the 16-bit result, which is never stored.

    With ``w_group_adapter`` (int32 [groups]) ``w`` holds ``n_adapters * n_per_adapter`` rows — the per-sample weight slots of
    the merged-LoRA mode stacked along the rows — and group g uses rows ``[id_g * n_per_adapter, (id_g + 1) * n_per_adapter)``."""
    M, K = a.rows, a.K
    assert w.K == K
    N = n_per_adapter if w_group_adapter is not None else w.rows
    n_out = N // 2 if act == L.ACT_GEGLU else N
    oq = None
    if out_mx8:
        assert act == L.ACT_GEGLU and N % 256 == 0
        oq = out        # a caller's Mx8Tensor (any row stride % 16, any scale stride >= M, % 4), as quant_mx8 takes one
        if oq is None:
            oq = Mx8Tensor(torch.empty((M, n_out), dtype=torch.uint8, device=a.q.device),
                           torch.empty((n_out // 128, (M + 3) // 4 * 4), dtype=torch.int32, device=a.q.device), tuple(a.shape[:-1]) + (n_out,))
        assert isinstance(oq, Mx8Tensor) and oq.scales.shape[0] == n_out // 128
        out = oq.q
    elif out is None:
        out = torch.empty((M, n_out), dtype=out_dtype, device=a.q.device)
    assert out.stride(1) == 1 and out.shape == (M, n_out)
    g = L.GemmMx8Args()
    g.dtype = _DT[out_dtype] if out_mx8 else _dt(out)
    g.M, g.N, g.K = M, N, K
    g.A, g.lda, g.a_scale, g.sa_ld = a.q.data_ptr(), a.q.stride(0), a.scales.data_ptr(), a.scales.stride(0)
    g.W, g.ldw, g.w_scale, g.sw_ld = w.q.data_ptr(), w.q.stride(0), w.scales.data_ptr(), w.scales.stride(0)
    g.groups, g.rows_per_group = groups, M // groups
    if w_group_adapter is not None:
        g.group_adapter = w_group_adapter.data_ptr()
        g.w_adapter_stride, g.sw_adapter_stride = N * w.q.stride(0), N
    g.bias = _p(bias)
    if residual is not None:
        assert residual.stride(1) == 1
        g.residual, g.ldr = residual.data_ptr(), residual.stride(0)
    g.act, g.out_scale = act, out_scale
    g.C, g.ldc = out.data_ptr(), out.stride(0)
    if oq is not None:
        g.c_scale, g.sc_ld = oq.scales.data_ptr(), oq.scales.stride(0)
    if _PROF is not None:
        t0 = _PROF.begin()
        L.check(L.lib().omg_gemm_mx8(C.byref(g), _stream()), "omg_gemm_mx8")
        _PROF.end("gemm_mx8", 2.0 * M * N * K, t0, ("mx8", M, N, K, 0, groups if w_group_adapter is not None else 1, act))
        return oq if oq is not None else out
    L.check(L.lib().omg_gemm_mx8(C.byref(g), _stream()), "omg_gemm_mx8")
    return oq if oq is not None else out


def conv2d(x1: torch.Tensor, w: torch.Tensor, ksize: int, *, stride: int = 1, upsample: "bool | int" = False,
           x2: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
           group_bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           out_scale: float = 1.0, act: int = L.ACT_NONE, w_group_adapter: Optional[torch.Tensor] = None,
           lora: Optional[LoraSpec] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NHWC implicit-GEMM conv; ``w`` is ``[Cout, ksize*ksize*(C1+C2)]`` (see pack_conv_weight).

    ``upsample``: False / True (the convolution of the nearest-2x upsampled input, all nine taps), or 2 — the same convolution as four
    2x2 phase convolutions on the source image (4/9 of the multiplies; ``w`` from :func:`pack_conv_weight_phase`; equal to
    ``upsample=True`` up to one rounding of the summed weights and the order of the fp32 accumulation).

    LoRA on convolutions (``omg_conv2d_slots``): ``w`` may be 3-D ``[slots, Cout, K]`` together with ``w_group_adapter`` (int32
    device tensor, one weight slot per sample; a sample with slot -1 is skipped and its rows of ``out`` stay as they are) — the
    merged-weight conv and the LoRA-down conv; ``lora`` adds ``a2 @ w2[slot]^T`` (``a2``: the down conv's result, 2-D or NHWC)
    into the accumulator of the samples whose slot is >= 0.  Without these arguments the call is ``omg_conv2d``, unchanged.
    ``out`` (optional, NHWC contiguous): write there instead of allocating — what makes "skipped rows stay as they are" observable
    (the canary test of the LoRA-down launch) and lets tools/conv_slots_bench.py time launches without the allocator.
    """
    _dev(x1)
    B, Hin, Win, C1 = x1.shape
    assert x1.is_contiguous()
    C2 = 0
    if x2 is not None:
        assert x2.is_contiguous() and x2.shape[:3] == x1.shape[:3]
        C2 = x2.shape[3]
    phase = int(upsample) == 2
    Cout = w.shape[-2]
    if phase:
        # the four 2x2 phase convolutions on the source image: ``w`` is pack_conv_weight_phase's [4, Cout, 4 * C1] ([slots, 4, Cout, 4 * C1])
        if ksize != 3 or stride != 1 or x2 is not None or lora is not None or residual is not None:
            raise L.OmgHipError("the phase form (upsample=2) is the 3x3 / stride 1 convolution of one input without residual or LoRA segment")
        assert w.is_contiguous() and w.dim() in (3, 4) and tuple(w.shape[-3:]) == (4, Cout, 4 * C1)
        slots = w.dim() == 4 or w_group_adapter is not None
    else:
        slots = w.dim() == 3 or w_group_adapter is not None or lora is not None
        assert w.is_contiguous() and w.shape[-1] == ksize * ksize * (C1 + C2)
    Hl, Wl = (2 * Hin, 2 * Win) if upsample else (Hin, Win)
    pad = 1 if ksize == 3 else 0
    Hout = (Hl + 2 * pad - ksize) // stride + 1
    Wout = (Wl + 2 * pad - ksize) // stride + 1
    if out is None:
        y = torch.empty((B, Hout, Wout, Cout), dtype=x1.dtype, device=x1.device)
    else:
        y = out
        assert y.is_contiguous() and tuple(y.shape) == (B, Hout, Wout, Cout) and y.dtype == x1.dtype
    sa = L.Conv2dSlotsArgs() if slots else None
    a = sa.conv if slots else L.Conv2dArgs()
    a.dtype = _dt(x1)
    a.B, a.Hin, a.Win, a.C1, a.C2 = B, Hin, Win, C1, C2
    a.Hout, a.Wout, a.Cout = Hout, Wout, Cout
    a.ksize, a.stride, a.upsample = ksize, stride, int(upsample)
    a.X1, a.X2, a.W, a.bias = x1.data_ptr(), _p(x2), w.data_ptr(), _p(bias)
    if group_bias is not None:
        a.group_bias, a.ldgb = group_bias.data_ptr(), group_bias.stride(0)
    if residual is not None:
        assert residual.is_contiguous() and residual.shape == y.shape
        a.residual = residual.data_ptr()
    a.out_scale = out_scale
    a.act = act
    a.Y = y.data_ptr()
    k2 = 0
    if slots:
        adapter = w_group_adapter
        sa.w_slot_stride = w.stride(0) if w.dim() == (4 if phase else 3) else 0
        if lora is not None:
            a2, w2 = lora.a2, lora.w2
            a2 = a2.reshape(-1, a2.shape[-1])
            assert a2.stride(1) == 1 and a2.shape[0] == B * Hout * Wout and w2.stride(-1) == 1 and w2.shape[-2] == Cout and lora.a2_col_block == 0
            k2 = w2.shape[-1]
            sa.A2, sa.lda2, sa.W2, sa.K2 = a2.data_ptr(), a2.stride(0), w2.data_ptr(), k2
            if w2.dim() == 3:
                sa.ldw2, sa.w2_slot_stride = w2.stride(1), w2.stride(0)
            else:
                sa.ldw2, sa.w2_slot_stride = w2.stride(0), 0
            if lora.group_adapter is not None:
                adapter = lora.group_adapter
        if adapter is not None:
            assert adapter.dtype == torch.int32 and adapter.is_cuda and adapter.numel() == B
        sa.group_adapter = _p(adapter)
        fn, what, arg = L.lib().omg_conv2d_slots, "omg_conv2d_slots", sa
    else:
        fn, what, arg = L.lib().omg_conv2d, "omg_conv2d", a
    if _PROF is not None:
        t0 = _PROF.begin()
        L.check(fn(C.byref(arg), _stream()), what)
        if phase:       # the executed work: the call's four launches of M = B Hin Win rows and K = 4 C1 in one record, under one launch's shape
            _PROF.end("gemm", 2.0 * 4 * B * Hin * Win * Cout * 4 * C1, t0, ("conv", B * Hin * Win, Cout, 4 * C1, 0, B if slots else 1, "x4 phases"))
            return y
        K = ksize * ksize * (C1 + C2)
        _PROF.end("gemm", 2.0 * B * Hout * Wout * Cout * (K + k2), t0, ("conv", B * Hout * Wout, Cout, K, k2, B if slots else 1, 0))
        return y
    L.check(fn(C.byref(arg), _stream()), what)
    return y


class Mx8Map:
    """An MX-fp8 NHWC feature map: ``q`` uint8 [B, H, W, Cq] (OCP e4m3), ``scales`` int32 [Cq/128, B*H*W] (byte j of a dword = the
    E8M0 scale of channels 128 k + 32 j .. + 31 of that pixel) — what omg_groupnorm_mx8 writes and omg_conv2d_mx8 reads.
    Cq = the channel count rounded up to a multiple of 128; pad channels are zeros."""

    __slots__ = ("q", "scales", "shape", "dtype")

    def __init__(self, q: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype):
        self.q, self.scales, self.shape, self.dtype = q, scales, tuple(q.shape), dtype

    @property
    def device(self):
        return self.q.device


def groupnorm_mx8(x1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, *,
                  silu: bool = False, x2: Optional[torch.Tensor] = None) -> Mx8Map:
    """NHWC GroupNorm (+SiLU) of [x1 | x2] straight into MX-fp8 (the input of an MX-fp8 convolution): equal to quantising
    :func:`groupnorm`'s 16-bit output, which is never stored."""
    _dev(x1)
    assert x1.is_contiguous() and x1.dim() == 4
    B, H, W, C1 = x1.shape
    C2 = 0
    if x2 is not None:
        assert x2.is_contiguous() and x2.shape[:3] == x1.shape[:3]
        C2 = x2.shape[-1]
    Cc = C1 + C2
    if Cc % 32 != 0:
        raise L.OmgHipError("MX-fp8 feature maps need C % 32 == 0")
    Cq = (Cc + 127) // 128 * 128
    out = Mx8Map(torch.empty((B, H, W, Cq), dtype=torch.uint8, device=x1.device),
                 torch.empty((Cq // 128, B * H * W), dtype=torch.int32, device=x1.device), x1.dtype)
    ws = _gn_workspace(x1.device, B, groups, H * W)
    assert gamma.dtype == x1.dtype and beta.dtype == x1.dtype
    L.check(L.lib().omg_groupnorm_mx8(_dt(x1), x1.data_ptr(), C1, _p(x2), C2, B, H * W, groups, eps, gamma.data_ptr(), beta.data_ptr(),
                                      int(silu), ws.data_ptr(), out.q.data_ptr(), out.scales.data_ptr(), _stream()), "omg_groupnorm_mx8")
    return out


def conv2d_mx8(x: Mx8Map, w: "Mx8Tensor", *, bias: Optional[torch.Tensor] = None, group_bias: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, out_scale: float = 1.0, act: int = L.ACT_NONE) -> torch.Tensor:
    """3x3 / stride 1 / pad 1 convolution on the block-scaled fp8 MFMA (omg_conv2d_mx8).  ``w`` = quant_mx8 of the packed
    [Cout, 9*Cin] weight (pack_conv_weight); output, bias, per-sample bias and residual in ``x.dtype``."""
    _dev(x.q)
    B, H, W, Cin = x.shape
    Cout = w.rows
    assert w.K == 9 * Cin
    y = torch.empty((B, H, W, Cout), dtype=x.dtype, device=x.device)
    a = L.Conv2dMx8Args()
    a.dtype = _DT[x.dtype]
    a.B, a.H, a.W, a.Cin, a.Cout = B, H, W, Cin, Cout
    a.X, a.x_scale, a.Wq, a.w_scale = x.q.data_ptr(), x.scales.data_ptr(), w.q.data_ptr(), w.scales.data_ptr()
    a.sw_ld, a.act = w.scales.stride(0), act
    a.bias = _p(bias)
    if group_bias is not None:
        a.group_bias, a.ldgb = group_bias.data_ptr(), group_bias.stride(0)
    if residual is not None:
        assert residual.is_contiguous() and residual.shape == y.shape and residual.dtype == y.dtype
        a.residual = residual.data_ptr()
    a.out_scale = out_scale
    a.Y = y.data_ptr()
    if _PROF is not None:
        t0 = _PROF.begin()
        L.check(L.lib().omg_conv2d_mx8(C.byref(a), _stream()), "omg_conv2d_mx8")
        _PROF.end("gemm_mx8", 2.0 * B * H * W * Cout * 9 * Cin, t0, ("conv_mx8", B * H * W, Cout, 9 * Cin, 0, 1, 0))
        return y
    L.check(L.lib().omg_conv2d_mx8(C.byref(a), _stream()), "omg_conv2d_mx8")
    return y


# which kernel the last conv2d_f32 call launched: "direct" (conv_f32_kernel) or "winograd" (conv_f32_wino_kernel)
LAST_CONV2D_F32_ALGO: Optional[str] = None
_F32_AUTO = {"winograd": True, "min_blocks": 256}


def set_conv2d_f32_auto(winograd: bool = True, min_blocks: int = 256) -> None:
    """What conv2d_f32(algo="auto") does: ``winograd=False`` keeps every launch on the direct kernel; ``min_blocks`` is the number of
    Winograd workgroups from which a launch counts as filling the machine (256 CUs; 0: Winograd wherever it applies)."""
    _F32_AUTO["winograd"], _F32_AUTO["min_blocks"] = bool(winograd), int(min_blocks)


def conv2d_f32(x: torch.Tensor, w: torch.Tensor, ksize: int, *, upsample: bool = False, bias: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, algo: str = "auto", wu: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 NHWC convolution on the f32-input MFMA: the up blocks of the upcast VAE decode.
    ``w``: fp32 [Cout, ksize*ksize*Cin] (pack_conv_weight of the fp32 OIHW tensor).  ``wu``: the Winograd image of the same weight
    (pack_conv_weight_wino).  ``algo``: "direct" = omg_conv2d_f32 (exact direct convolution), "winograd" = omg_conv2d_f32_wino
    (F(2x2, 3x3); needs ``wu``, ksize 3, even output sizes, Cin % 8 == 0 — an error otherwise), "auto" = Winograd where it applies and
    the launch fills the machine (at least one 16 x 16 x 64 block per CU), else direct.  ``out``: a contiguous fp32 tensor of the
    output's shape to write into (must not alias ``x``)."""
    global LAST_CONV2D_F32_ALGO
    _dev(x)
    assert x.dtype == torch.float32 and w.dtype == torch.float32 and x.is_contiguous() and w.is_contiguous()
    assert algo in ("auto", "direct", "winograd")
    B, Hin, Win, Cin = x.shape
    Cout = w.shape[0]
    assert w.shape[1] == ksize * ksize * Cin
    Ho, Wo = (2 * Hin, 2 * Win) if upsample else (Hin, Win)
    wino_ok = ksize == 3 and Ho % 2 == 0 and Wo % 2 == 0 and Cin % 8 == 0 and wu is not None
    if algo == "winograd" and not wino_ok:
        raise L.OmgHipError("conv2d_f32(algo='winograd') needs ksize 3, even output sizes, Cin % 8 == 0 and the wu weight image")
    use_wino = algo == "winograd" or (algo == "auto" and wino_ok and _F32_AUTO["winograd"]
                                      and B * ((Ho + 15) // 16) * ((Wo + 15) // 16) * ((Cout + 63) // 64) >= _F32_AUTO["min_blocks"])
    if out is None:
        y = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    else:
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (B, Ho, Wo, Cout) and out.device == x.device
        y = out
    if bias is not None:
        assert bias.dtype == torch.float32
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.is_contiguous() and residual.shape == y.shape
    if use_wino:
        assert wu.dtype == torch.float32 and wu.is_contiguous() and wu.device == x.device
        assert wu.numel() == L.lib().omg_conv2d_f32_wino_weight_floats(Cout, Cin)
        a = L.Conv2dF32WinoArgs()
        a.B, a.Hin, a.Win, a.Cin, a.Hout, a.Wout, a.Cout, a.upsample = B, Hin, Win, Cin, Ho, Wo, Cout, int(upsample)
        a.X, a.U, a.Y = x.data_ptr(), wu.data_ptr(), y.data_ptr()
        fn, name, tag = L.lib().omg_conv2d_f32_wino, "omg_conv2d_f32_wino", "conv_f32_wino"
        flops = 2.0 * B * Ho * Wo * Cout * 4 * Cin          # executed matrix FLOPs: 16 products per 2x2 tile and (cin, cout) = 16/36 of direct
    else:
        a = L.Conv2dF32Args()
        a.B, a.Hin, a.Win, a.Cin, a.Hout, a.Wout, a.Cout, a.ksize, a.upsample = B, Hin, Win, Cin, Ho, Wo, Cout, ksize, int(upsample)
        a.X, a.W, a.Y = x.data_ptr(), w.data_ptr(), y.data_ptr()
        fn, name, tag = L.lib().omg_conv2d_f32, "omg_conv2d_f32", "conv_f32"
        flops = 2.0 * B * Ho * Wo * Cout * ksize * ksize * Cin
    a.bias, a.residual = _p(bias), _p(residual)
    LAST_CONV2D_F32_ALGO = "winograd" if use_wino else "direct"
    if _PROF is not None:
        t0 = _PROF.begin()
        L.check(fn(C.byref(a), _stream()), name)
        _PROF.end("gemm_f32", flops, t0, (tag, B * Ho * Wo, Cout, ksize * ksize * Cin, 0, 1, 0))
        return y
    L.check(fn(C.byref(a), _stream()), name)
    return y


def cast_f32(x: torch.Tensor) -> torch.Tensor:
    """16-bit -> fp32 copy (same shape / layout)."""
    _dev(x)
    assert x.is_contiguous() and x.numel() % 8 == 0
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.check(L.lib().omg_cast_f32(_dt(x), x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "omg_cast_f32")
    return y


def transpose_v(v: torch.Tensor, heads: int, nkv_pad: Optional[int] = None, out: Optional[torch.Tensor] = None,
                mfma_order: bool = True) -> torch.Tensor:
    """``v``: (B, Nkv, >=heads*64) view with unit inner stride -> Vt (B, heads, 64, Nkv_pad).  ``mfma_order`` (default): the key
    order :func:`attention` consumes ([0-3, 8-11, 4-7, 12-15] inside every 16 keys); False: a plain transpose."""
    _dev(v)
    B, Nkv = v.shape[0], v.shape[1]
    if nkv_pad is None:
        nkv_pad = (Nkv + 63) // 64 * 64
    vt = out if out is not None else torch.empty((B, heads, 64, nkv_pad), dtype=v.dtype, device=v.device)
    assert vt.is_contiguous() and tuple(vt.shape) == (B, heads, 64, nkv_pad)
    L.check(L.lib().omg_transpose_v(_dt(v), v.data_ptr(), v.stride(1), v.stride(0), B, heads, Nkv, nkv_pad,
                                    vt.data_ptr(), int(mfma_order), _stream()), "omg_transpose_v")
    return vt


def transpose_v_mapped(v: torch.Tensor, heads: int, edit_of: torch.Tensor, mapper: torch.Tensor, alpha: torch.Tensor,
                       step_idx: Optional[torch.Tensor] = None, nkv_pad: Optional[int] = None,
                       out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two V^T images of a general prompt-to-prompt cross edit (omg_transpose_v_mapped), one launch for the batch.

    ``v``: (B, Nkv <= 128, >= heads*64) view with unit inner stride; ``edit_of``: int32 (B,) table index per row, -1 = not edited;
    ``mapper``: fp32 (E, >= Nkv, >= Nkv); ``alpha``: fp32 (steps, E, >= Nkv); ``step_idx``: device int32 scalar selecting the alpha row
    (None = row 0).  Returns (Vt_mapped, Vt_own), each (B, heads, 64, nkv_pad) in :func:`transpose_v`'s MFMA key order; pass ``out`` to
    write into existing buffers (pointer-stable across steps for captured graphs)."""
    _dev(v)
    B, Nkv = v.shape[0], v.shape[1]
    if nkv_pad is None:
        nkv_pad = (Nkv + 63) // 64 * 64
    assert v.stride(2) == 1
    assert edit_of.dtype == torch.int32 and edit_of.is_contiguous() and edit_of.numel() == B and edit_of.device == v.device
    assert mapper.dtype == torch.float32 and mapper.dim() == 3 and mapper.stride(2) == 1 and mapper.device == v.device
    assert alpha.dtype == torch.float32 and alpha.dim() == 3 and alpha.stride(2) == 1 and alpha.device == v.device
    assert alpha.shape[1] == mapper.shape[0]
    if mapper.shape[1] < Nkv or alpha.shape[2] < Nkv:
        raise L.OmgHipError(f"transpose_v_mapped: tables cover {min(mapper.shape[1], alpha.shape[2])} keys, V has {Nkv}")
    if out is None:
        out = (torch.empty((B, heads, 64, nkv_pad), dtype=v.dtype, device=v.device),
               torch.empty((B, heads, 64, nkv_pad), dtype=v.dtype, device=v.device))
    vm, vo = out
    for t in (vm, vo):
        assert t.is_contiguous() and tuple(t.shape) == (B, heads, 64, nkv_pad) and t.dtype == v.dtype
    a = L.VMapArgs()
    a.dtype, a.B, a.heads, a.Nkv, a.Nkv_pad = _dt(v), B, heads, Nkv, nkv_pad
    a.V, a.ldv, a.v_bstride = v.data_ptr(), v.stride(1), v.stride(0)
    a.edit_of, a.E, a.steps = edit_of.data_ptr(), mapper.shape[0], alpha.shape[0]
    a.mapper, a.ld_mapper, a.mapper_estride = mapper.data_ptr(), mapper.stride(1), mapper.stride(0)
    a.alpha, a.alpha_step_stride, a.alpha_estride = alpha.data_ptr(), alpha.stride(0), alpha.stride(1)
    if step_idx is not None:
        assert step_idx.dtype == torch.int32 and step_idx.device == v.device
        a.step_idx = step_idx.data_ptr()
    a.Vt_mapped, a.Vt_own = vm.data_ptr(), vo.data_ptr()
    L.check(L.lib().omg_transpose_v_mapped(C.byref(a), _stream()), "omg_transpose_v_mapped")
    return vm, vo


class RowMajorV:
    """The V operand of a self-attention as the QKV projection wrote it — a (B, Nkv, heads*64) VIEW with unit inner stride — instead of the
    V^T image :func:`transpose_v` makes: :func:`attention` hands it to the kernel that transposes on the LDS read (omg_attn_args.V, ABI 6).
    More than 128 keys only (:func:`value_operand` chooses)."""

    def __init__(self, v: torch.Tensor):
        assert v.dim() == 3 and v.stride(2) == 1 and v.stride(1) % 8 == 0 and v.stride(0) % 8 == 0 and v.shape[1] > 128
        self.v = v


def value_operand(v: torch.Tensor, heads: int):
    """What :func:`attention` wants for ``v`` (B, Nkv, heads*64): the view itself above 128 keys when its strides allow (self-attention
    at 32 x 32 / 64 x 64), else the V^T image in MFMA key order."""
    if v.shape[1] > 128 and v.stride(2) == 1 and v.stride(1) % 8 == 0 and v.stride(0) % 8 == 0 and v.data_ptr() % 16 == 0:
        return RowMajorV(v)
    return transpose_v(v, heads)


def _attn_args(q, k, vt, heads, nkv, scale, qk_src, out, accumulate, out_scale) -> L.AttnArgs:
    a = L.AttnArgs()
    a.dtype = _dt(q)
    a.B, a.heads, a.Nq, a.Nkv = q.shape[0], heads, q.shape[1], nkv
    a.Q, a.ldq, a.q_bstride = q.data_ptr(), q.stride(1), q.stride(0)
    a.K, a.ldk, a.k_bstride = k.data_ptr(), k.stride(1), k.stride(0)
    if isinstance(vt, RowMajorV):
        a.V, a.ldv, a.v_bstride = vt.v.data_ptr(), vt.v.stride(1), vt.v.stride(0)
    elif vt is not None:
        a.Vt, a.Nkv_pad = vt.data_ptr(), vt.shape[3]
    a.qk_src = _p(qk_src)
    a.scale = scale
    a.accumulate = int(accumulate)
    a.out_scale = out_scale
    if out is not None:
        a.O, a.ldo, a.o_bstride = out.data_ptr(), out.stride(1), out.stride(0)
    return a


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, scale: float, *,
              qk_src: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              accumulate: bool = False, out_scale: float = 1.0, causal: bool = False) -> torch.Tensor:
    """Fused attention.  q: (B,Nq,>=heads*64) view, k: (B,Nkv,>=heads*64) view, vt from :func:`value_operand` (or transpose_v).

    ``qk_src`` (int32 device tensor [B]) implements the controller's probability replacement:
    sample b uses Q,K of sample qk_src[b] and its own V.

    ``causal``: query i sees keys j <= i only (top-left alignment; `omg_attn_fwd_causal`: at most 128 keys, ``vt`` from
    :func:`transpose_v` in its default key order; anything else is an error, not another path).
    """
    _dev(q)
    assert q.stride(2) == 1 and k.stride(2) == 1
    B, Nq = q.shape[0], q.shape[1]
    if out is None:
        out = torch.empty((B, Nq, heads * 64), dtype=q.dtype, device=q.device)
    a = _attn_args(q, k, vt, heads, k.shape[1], scale, qk_src, out, accumulate, out_scale)
    fn, what = (L.lib().omg_attn_fwd_causal, "omg_attn_fwd_causal") if causal else (L.lib().omg_attn_fwd, "omg_attn_fwd")
    if _PROF is not None:
        t0 = _PROF.begin()
        L.check(fn(C.byref(a), _stream()), what)
        _PROF.end("attn", 4.0 * B * heads * Nq * k.shape[1] * 64, t0, ("attn", B, heads, Nq, k.shape[1]))
        return out
    L.check(fn(C.byref(a), _stream()), what)
    return out


def attn_probs(q: torch.Tensor, k: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """Materialised softmax probabilities (B*heads, Nq, Nkv) — protocol mode only."""
    _dev(q)
    B, Nq, Nkv = q.shape[0], q.shape[1], k.shape[1]
    p = torch.empty((B * heads, Nq, Nkv), dtype=q.dtype, device=q.device)
    a = _attn_args(q, k, None, heads, Nkv, scale, None, None, False, 1.0)
    L.check(L.lib().omg_attn_probs(C.byref(a), p.data_ptr(), _stream()), "omg_attn_probs")
    return p


def attn_apply_probs(p: torch.Tensor, v: torch.Tensor, heads: int) -> torch.Tensor:
    _dev(p)
    B, Nkv = v.shape[0], v.shape[1]
    Nq = p.shape[1]
    assert p.is_contiguous() and p.shape[0] == B * heads and p.shape[2] == Nkv
    out = torch.empty((B, Nq, heads * 64), dtype=p.dtype, device=p.device)
    L.check(L.lib().omg_attn_apply_probs(_dt(p), p.data_ptr(), v.data_ptr(), v.stride(1), v.stride(0), B, heads, Nq,
                                         Nkv, out.data_ptr(), out.stride(1), out.stride(0), _stream()),
            "omg_attn_apply_probs")
    return out


def _gn_workspace(device, B: int, groups: int, HW: int) -> torch.Tensor:
    """Partial-sum scratch of one GroupNorm call.  Allocated PER CALL: a module-level buffer that grew on demand was, under
    hipGraph capture, born in the capturing engine's private pool — a graph of ANOTHER engine captured later kept the pointer, and
    when the first engine dropped its graphs (pointer epoch) the block was unmapped under the survivor's replay (memory access
    fault in a stage 1 -> stage 2 sequence at full size, round 3).  Inside a capture torch gives every call its own slot of the
    graph's pool; outside, the caching allocator makes this a free-list lookup."""
    n = int(L.lib().omg_groupnorm_ws_floats(B, groups, HW))
    return torch.empty(max(n, 1), dtype=torch.float32, device=device)


def groupnorm(x1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, *,
              silu: bool = False, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NHWC GroupNorm (+SiLU) of the channel-concat [x1 | x2]; x: (B, H, W, C) or (B, HW, C)."""
    _dev(x1)
    assert x1.is_contiguous()
    B = x1.shape[0]
    C1 = x1.shape[-1]
    HW = x1.numel() // (B * C1)
    C2 = 0
    if x2 is not None:
        assert x2.is_contiguous()
        C2 = x2.shape[-1]
    y = torch.empty(x1.shape[:-1] + (C1 + C2,), dtype=x1.dtype, device=x1.device)
    ws = _gn_workspace(x1.device, B, groups, HW)
    assert gamma.dtype == x1.dtype and beta.dtype == x1.dtype
    L.check(L.lib().omg_groupnorm(_dt(x1, allow_f32=True), x1.data_ptr(), C1, _p(x2), C2, B, HW, groups, eps, gamma.data_ptr(),
                                  beta.data_ptr(), int(silu), ws.data_ptr(), y.data_ptr(), _stream()), "omg_groupnorm")
    return y


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    _dev(x)
    Cc = x.shape[-1]
    x2 = x.reshape(-1, Cc)
    assert x2.stride(1) == 1
    y = torch.empty((x2.shape[0], Cc), dtype=x.dtype, device=x.device)
    L.check(L.lib().omg_layernorm(_dt(x), x2.data_ptr(), x2.stride(0), x2.shape[0], Cc, eps, gamma.data_ptr(),
                                  beta.data_ptr(), y.data_ptr(), y.stride(0), _stream()), "omg_layernorm")
    return y.view(x.shape)


def layernorm_mx8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> "Mx8Tensor":
    """LayerNorm straight into MX-fp8 (bytes + block scales): the input of an MX-fp8 Linear; rows = all leading dims."""
    _dev(x)
    Cc = x.shape[-1]
    x2 = x.reshape(-1, Cc)
    assert x2.stride(1) == 1
    M = x2.shape[0]
    out = Mx8Tensor(torch.empty((M, Cc), dtype=torch.uint8, device=x.device),
                    torch.empty((Cc // 128, (M + 3) // 4 * 4), dtype=torch.int32, device=x.device), x.shape)
    L.check(L.lib().omg_layernorm_mx8(_dt(x), x2.data_ptr(), x2.stride(0), M, Cc, eps, gamma.data_ptr(), beta.data_ptr(),
                                      out.q.data_ptr(), out.q.stride(0), out.scales.data_ptr(), out.scales.stride(0), _stream()),
            "omg_layernorm_mx8")
    return out


def dwconv2d(x: torch.Tensor, taps: torch.Tensor, B: int, H: int, W: int, ksize: int, bias: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise ``ksize x ksize`` convolution (stride 1, same padding) of NHWC rows ``x`` [B*H*W, C] (any row stride: a column slice
    of a wider buffer is fine); ``taps`` [ksize*ksize, C] tap-major; ``out`` [B*H*W, C] with any row stride, not overlapping ``x``.
    omg_dwconv2d — LiteMLA's multi-scale aggregation."""
    _dev(x)
    M, Cc = x.shape
    assert M == B * H * W and x.stride(1) == 1 and taps.shape == (ksize * ksize, Cc) and taps.is_contiguous() and taps.dtype == x.dtype
    if bias is not None:
        assert bias.shape == (Cc,) and bias.is_contiguous() and bias.dtype == x.dtype and bias.device == x.device
    if out is None:
        y = torch.empty((M, Cc), dtype=x.dtype, device=x.device)
    else:
        y = out
        assert y.shape == (M, Cc) and y.stride(1) == 1 and y.dtype == x.dtype and y.device == x.device
        es = x.element_size()
        x0, y0 = x.data_ptr(), y.data_ptr()
        if M and x0 < y0 + ((M - 1) * y.stride(0) + Cc) * es and y0 < x0 + ((M - 1) * x.stride(0) + Cc) * es:
            # the same buffer: the same rows, and columns that x does not have
            dcol = abs(y0 - x0) // es % max(x.stride(0), 1)
            assert x.stride(0) == y.stride(0) and Cc <= dcol <= x.stride(0) - Cc, "dwconv2d: out overlaps x"
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_dwconv2d(_dt(x), x.data_ptr(), x.stride(0), B, H, W, Cc, ksize, taps.data_ptr(), _p(bias), y.data_ptr(), y.stride(0), _stream()),
            "omg_dwconv2d")
    if _PROF is not None:
        _PROF.end("dwconv2d", 2.0 * M * Cc * ksize * ksize, t0, ("dwconv2d", M, Cc, ksize))
    return y


def litemla_aggreg(x: torch.Tensor, taps: torch.Tensor, wg: torch.Tensor, B: int, H: int, W: int, ksize: int, dim: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One scale of LiteMLA's aggregation in one launch: the depthwise ``ksize x ksize`` convolution of ``dwconv2d`` (rounded once to
    the storage dtype) and the 1x1 convolution with ``C / dim`` groups behind it.  ``x`` [B*H*W, C] NHWC rows (any row stride);
    ``taps`` [ksize*ksize, C]; ``wg`` [C, dim], the grouped convolution's own weight; ``out`` may be another column slice of the buffer
    ``x`` is a slice of.  dim 16 | 32.  omg_litemla_aggreg."""
    _dev(x)
    M, Cc = x.shape
    assert M == B * H * W and x.stride(1) == 1 and taps.shape == (ksize * ksize, Cc) and taps.is_contiguous()
    assert wg.shape == (Cc, dim) and wg.is_contiguous() and taps.dtype == x.dtype and wg.dtype == x.dtype
    if out is None:
        out = torch.empty((M, Cc), dtype=x.dtype, device=x.device)
    assert out.shape == (M, Cc) and out.stride(1) == 1 and out.dtype == x.dtype and out.device == x.device
    es = x.element_size()
    x0, y0 = x.data_ptr(), out.data_ptr()
    if M and x0 < y0 + ((M - 1) * out.stride(0) + Cc) * es and y0 < x0 + ((M - 1) * x.stride(0) + Cc) * es:
        # the same buffer: the same rows, and columns that x does not have
        dcol = abs(y0 - x0) // es % max(x.stride(0), 1)
        assert x.stride(0) == out.stride(0) and Cc <= dcol <= x.stride(0) - Cc, "litemla_aggreg: out overlaps x"
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_litemla_aggreg(_dt(x), x0, x.stride(0), B, H, W, Cc, ksize, dim, taps.data_ptr(), wg.data_ptr(), y0, out.stride(0),
                                       _stream()), "omg_litemla_aggreg")
    if _PROF is not None:
        _PROF.end("litemla_aggreg", 2.0 * M * Cc * (ksize * ksize + dim), t0, ("litemla_aggreg", M, Cc, ksize, dim))
    return out


def relu_linear_att(qkv: torch.Tensor, B: int, HW: int, groups: int, dim: int, eps: float, out: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """EfficientViT's ReLU linear attention (fp32 inside) on NHWC rows ``qkv`` [B*HW, groups*3*dim] (group g: q | k | v at columns
    3 dim g; any row stride) -> [B*HW, groups*dim].  ``out`` may have any row stride and must not overlap ``qkv``; ``workspace`` is a
    contiguous fp32 tensor of at least omg_relu_linear_att_ws_floats elements, every one of which the call writes before it reads it.
    omg_relu_linear_att."""
    _dev(qkv)
    M, Cc = qkv.shape
    assert M == B * HW and Cc == groups * 3 * dim and qkv.stride(1) == 1
    if out is None:
        out = torch.empty((M, groups * dim), dtype=qkv.dtype, device=qkv.device)
    else:
        assert out.shape == (M, groups * dim) and out.stride(1) == 1 and out.dtype == qkv.dtype and out.device == qkv.device
        es = qkv.element_size()
        x0, y0 = qkv.data_ptr(), out.data_ptr()
        assert not (M and x0 < y0 + ((M - 1) * out.stride(0) + groups * dim) * es and y0 < x0 + ((M - 1) * qkv.stride(0) + Cc) * es), \
            "relu_linear_att: out overlaps qkv"
    need = int(L.lib().omg_relu_linear_att_ws_floats(B, groups, dim, HW))
    if workspace is None:
        ws = torch.empty((need,), dtype=torch.float32, device=qkv.device)
    else:
        ws = workspace
        assert ws.dtype == torch.float32 and ws.device == qkv.device and ws.dim() == 1 and ws.is_contiguous() and ws.numel() >= need
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_relu_linear_att(_dt(qkv), qkv.data_ptr(), qkv.stride(0), B, HW, groups, dim, eps, ws.data_ptr(), out.data_ptr(), out.stride(0),
                                        _stream()), "omg_relu_linear_att")
    if _PROF is not None:
        _PROF.end("relu_linear_att", 4.0 * M * groups * dim * (dim + 1), t0, ("relu_linear_att", M, groups, dim))
    return out


def conv3x3_nhwc_act(x: torch.Tensor, w: torch.Tensor, *, stride: int = 1, bias: Optional[torch.Tensor] = None, gelu: bool = False,
                     residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense 3x3 convolution (padding 1, stride 1 | 2) of NHWC ``x`` [B, H, W, Cin] with ``w`` [Cout, 3, 3, Cin] (any Cin that is a
    multiple of 8, or below 8) -> [B, Hout, Wout, Cout]; bias, tanh GELU and residual in the epilogue.  omg_conv3x3_nhwc_act."""
    _dev(x)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and w.shape == (Cout, 3, 3, Cin) and w.dtype == x.dtype
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    assert out.shape == (B, Ho, Wo, Cout) and out.is_contiguous() and out.dtype == x.dtype
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous() and residual.dtype == x.dtype
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_conv3x3_nhwc_act(_dt(x), x.data_ptr(), B, H, W, Cin, Cout, stride, w.data_ptr(), _p(bias), int(gelu), _p(residual),
                                         out.data_ptr(), _stream()), "omg_conv3x3_nhwc_act")
    if _PROF is not None:
        _PROF.end("conv3x3_nhwc", 2.0 * B * Ho * Wo * Cout * 9 * Cin, t0, ("conv3x3_nhwc", B * Ho * Wo, Cout, 9 * Cin, stride))
    return out


def dwconv3x3_act(x: torch.Tensor, taps: torch.Tensor, B: int, H: int, W: int, *, stride: int = 1, bias: Optional[torch.Tensor] = None,
                  gelu: bool = False, gelu_in: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise 3x3 convolution (padding 1, stride 1 | 2) of NHWC rows ``x`` [B*H*W, C]; ``taps`` [9, C] tap-major.  ``gelu`` acts on
    the output, ``gelu_in`` on the input as it is read.  -> [B*Hout*Wout, C]; ``out``, if given, is that many rows of any stride >= C
    that is a multiple of 8 (a column slice of a wider buffer), not overlapping ``x``.  omg_dwconv3x3_act."""
    _dev(x)
    M, Cc = x.shape
    assert M == B * H * W and x.stride(1) == 1 and taps.shape == (9, Cc) and taps.is_contiguous()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        y = torch.empty((B * Ho * Wo, Cc), dtype=x.dtype, device=x.device)
    else:
        y = out
        assert y.dim() == 2 and y.shape == (B * Ho * Wo, Cc) and y.dtype == x.dtype and y.device == x.device
        assert y.stride(1) == 1 and (y.shape[0] <= 1 or (y.stride(0) >= Cc and y.stride(0) % 8 == 0)), "dwconv3x3_act: out row stride"
        es, x0, y0, My = x.element_size(), x.data_ptr(), y.data_ptr(), y.shape[0]
        if M and My and x0 < y0 + ((My - 1) * y.stride(0) + Cc) * es and y0 < x0 + ((M - 1) * x.stride(0) + Cc) * es:
            # the same buffer: rows of the same stride, and columns that x does not have
            dcol = abs(y0 - x0) // es % max(x.stride(0), 1)
            assert x.stride(0) == y.stride(0) and Cc <= dcol <= x.stride(0) - Cc, "dwconv3x3_act: out overlaps x"
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_dwconv3x3_act(_dt(x), x.data_ptr(), x.stride(0), B, H, W, Cc, stride, taps.data_ptr(), _p(bias),
                                      int(gelu) | (int(gelu_in) << 1), y.data_ptr(), y.stride(0) if y.shape[0] > 1 else Cc, _stream()),
            "omg_dwconv3x3_act")
    if _PROF is not None:
        _PROF.end("dwconv3x3", 2.0 * B * Ho * Wo * Cc * 9, t0, ("dwconv3x3", B * Ho * Wo, Cc, stride))
    return y


def upsample_add_nhwc(x: torch.Tensor, out: torch.Tensor, accumulate: bool = True) -> torch.Tensor:
    """``out`` [B, Hout, Wout, C] (+)= bicubic resize (align_corners=False) of NHWC ``x`` [B, Hin, Win, C].  omg_upsample_add_nhwc."""
    _dev(x)
    B, H, W, Cc = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.shape[0] == B and out.shape[3] == Cc and out.dtype == x.dtype
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_upsample_add_nhwc(_dt(x), x.data_ptr(), B, H, W, Cc, out.shape[1], out.shape[2], int(accumulate), out.data_ptr(),
                                          _stream()), "omg_upsample_add_nhwc")
    if _PROF is not None:
        _PROF.end("upsample_add", 32.0 * out.numel(), t0, ("upsample_add", H, W, Cc))
    return out


def attn_small(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``softmax(q k^T scale) v`` per head for head_dim 16 | 32: ``q`` [B, Nq, heads*d], ``k`` / ``v`` [B, Nk, heads*d] -> [B, Nq, heads*d].
    Any row / batch stride that is a multiple of 8 (a column slice of a projection buffer is fine).  omg_attn_small."""
    _dev(q)
    B, Nq, Wd = q.shape
    Nk = k.shape[1]
    assert k.shape == (B, Nk, Wd) and v.shape == (B, Nk, Wd) and Wd % heads == 0 and k.dtype == q.dtype and v.dtype == q.dtype
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    if out is None:
        out = torch.empty((B, Nq, Wd), dtype=q.dtype, device=q.device)
    assert out.shape == (B, Nq, Wd) and out.stride(2) == 1 and out.dtype == q.dtype
    L.check(L.lib().omg_attn_small(_dt(q), B, heads, Wd // heads, Nq, Nk, q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0),
                                   v.data_ptr(), v.stride(1), v.stride(0), scale, out.data_ptr(), out.stride(1), out.stride(0), _stream()),
            "omg_attn_small")
    return out


def pack_convt2x2_weight(w_iohw: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d weight [Cin, Cout, 2, 2] -> the GEMM operand [(dy, dx, cout), cin] of :func:`convt2x2_ln_gelu`."""
    cin, cout = w_iohw.shape[:2]
    assert w_iohw.shape[2:] == (2, 2)
    return w_iohw.permute(2, 3, 1, 0).reshape(4 * cout, cin).contiguous()


def convt2x2_ln_gelu(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor] = None, *, ln_weight: Optional[torch.Tensor] = None,
                     ln_bias: Optional[torch.Tensor] = None, eps: float = 1e-6, gelu: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``act(LN?(ConvTranspose2d(k=2, s=2)(x)))`` of NHWC ``x`` [B, H, W, Cin] -> [B, 2H, 2W, Cout]: omg_gemm against ``w_packed``
    (:func:`pack_convt2x2_weight`), then omg_convt2x2_ln_gelu (scatter, bias, per-pixel LayerNorm over channels, erf GELU)."""
    _dev(x)
    B, H, W, Cin = x.shape
    Cout = w_packed.shape[0] // 4
    assert x.is_contiguous() and w_packed.shape == (4 * Cout, Cin) and w_packed.dtype == x.dtype
    g = gemm(x.view(B * H * W, Cin), w_packed)
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W, Cout), dtype=x.dtype, device=x.device)
    assert out.shape == (B, 2 * H, 2 * W, Cout) and out.is_contiguous() and out.dtype == x.dtype
    L.check(L.lib().omg_convt2x2_ln_gelu(_dt(x), g.data_ptr(), g.stride(0), B, H, W, Cout, _p(bias), _p(ln_weight), _p(ln_bias), eps, int(gelu),
                                         out.data_ptr(), _stream()), "omg_convt2x2_ln_gelu")
    return out


def sam_mask_logits(hyper: torch.Tensor, up: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``logits[b, m, y, x] = sum_c hyper[b, m, c] up[b, y, x, c]`` in fp32: ``hyper`` [B, M <= 4, C], NHWC ``up`` [B, H, W, C].
    omg_sam_mask_logits."""
    _dev(up)
    B, H, W, Cc = up.shape
    M = hyper.shape[1]
    assert hyper.shape == (B, M, Cc) and hyper.is_contiguous() and up.is_contiguous() and hyper.dtype == up.dtype
    if out is None:
        out = torch.empty((B, M, H, W), dtype=torch.float32, device=up.device)
    assert out.shape == (B, M, H, W) and out.is_contiguous() and out.dtype == torch.float32
    L.check(L.lib().omg_sam_mask_logits(_dt(up), hyper.data_ptr(), up.data_ptr(), B, M, H * W, Cc, out.data_ptr(), _stream()), "omg_sam_mask_logits")
    return out


def sam_postprocess(low: torch.Tensor, image_size: int, input_size: Tuple[int, int], original_size: Tuple[int, int], *,
                    threshold: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SAM's postprocess_masks on fp32 ``low`` [B, M, Hl, Wl]: bilinear to ``image_size``², crop to ``input_size``, bilinear to
    ``original_size``.  ``threshold`` None -> fp32 logits; a number -> uint8 0 / 1 (logit > threshold).  omg_sam_postprocess."""
    _dev(low)
    if low.dtype != torch.float32:
        raise L.OmgHipError(f"sam_postprocess takes float32 logits, not {low.dtype}")
    B, M, Hl, Wl = low.shape
    oh, ow = int(original_size[0]), int(original_size[1])
    assert low.is_contiguous()
    u8 = threshold is not None
    if out is None:
        out = torch.empty((B, M, oh, ow), dtype=torch.uint8 if u8 else torch.float32, device=low.device)
    assert out.shape == (B, M, oh, ow) and out.is_contiguous() and out.dtype == (torch.uint8 if u8 else torch.float32)
    L.check(L.lib().omg_sam_postprocess(low.data_ptr(), B * M, Hl, Wl, int(image_size), int(input_size[0]), int(input_size[1]), oh, ow,
                                        float(threshold) if u8 else 0.0, int(u8), out.data_ptr(), _stream()), "omg_sam_postprocess")
    return out


def relu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``max(x, 0)`` of a contiguous tensor whose size is a multiple of 8 (``out=x`` for in place).  omg_relu."""
    _dev(x)
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.is_contiguous() and out.shape == x.shape and out.dtype == x.dtype
    L.check(L.lib().omg_relu(_dt(x), x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "omg_relu")
    return out


def attn_relpos(qkv: torch.Tensor, B: int, H: int, W: int, heads: int, rel_h: torch.Tensor, rel_w: torch.Tensor, scale: float, *,
                window: int = 0, pad_kv: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Softmax attention per head with SAM's decomposed relative-position bias on the fused projection ``qkv`` [B*H*W, 3*heads*d]
    (rows in image order, columns q | k | v, head-major; any row stride that is a multiple of 8) -> [B*H*W, heads*d]; d = 64 | 80.
    ``window`` 0: global, ``rel_h`` [2H-1, d], ``rel_w`` [2W-1, d].  ``window`` S: the S x S windows from the top left, tables
    [2S-1, d]; positions beyond the grid are keys with k | v = ``pad_kv`` [2*heads*d] (None: zeros).  omg_attn_relpos."""
    _dev(qkv)
    M, Wd = qkv.shape
    assert M == B * H * W and Wd % (3 * heads) == 0 and qkv.stride(1) == 1
    d = Wd // (3 * heads)
    S = (window, window) if window else (H, W)
    for name, t, n in (("rel_h", rel_h, S[0]), ("rel_w", rel_w, S[1])):
        if tuple(t.shape) != (2 * n - 1, d):
            raise L.OmgHipError(f"attn_relpos: {name} is {tuple(t.shape)}, the layer needs ({2 * n - 1}, {d}) (no interpolation of the table)")
        assert t.is_contiguous() and t.dtype == qkv.dtype and t.is_cuda
    if pad_kv is not None:
        assert pad_kv.shape == (2 * heads * d,) and pad_kv.is_contiguous() and pad_kv.dtype == qkv.dtype and pad_kv.is_cuda
    if out is None:
        out = torch.empty((M, heads * d), dtype=qkv.dtype, device=qkv.device)
    assert out.shape == (M, heads * d) and out.stride(1) == 1 and out.dtype == qkv.dtype
    L.check(L.lib().omg_attn_relpos(_dt(qkv), B, H, W, heads, d, window, qkv.data_ptr(), qkv.stride(0), rel_h.data_ptr(), rel_w.data_ptr(),
                                    _p(pad_kv), scale, out.data_ptr(), out.stride(0), _stream()), "omg_attn_relpos")
    return out


def gelu_erf(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """erf GELU (``nn.GELU()``) of a contiguous tensor whose size is a multiple of 8 (``out=x`` for in place).  omg_gelu_erf."""
    _dev(x)
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.is_contiguous() and out.shape == x.shape and out.dtype == x.dtype
    L.check(L.lib().omg_gelu_erf(_dt(x), x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "omg_gelu_erf")
    return out


def attn_swin(qkv: torch.Tensor, B: int, H: int, W: int, heads: int, table: torch.Tensor, scale: float, *, window: int, shift: int = 0,
              pad_kv: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Swin's (shifted-)window attention on the fused projection ``qkv`` [B*H*W, 3*heads*32] (rows in image order, columns q | k | v,
    head-major; any row stride that is a multiple of 8) -> [B*H*W, heads*32].  ``window`` S = 7 | 12, ``shift`` 0 | S // 2; ``table``
    [(2S-1)^2, heads] is the checkpoint's relative_position_bias_table; positions beyond the grid are keys with k | v = ``pad_kv``
    [2*heads*32] (None: zeros).  Pad, roll, partition, bias, mask and reverse happen inside the kernel.  omg_attn_swin."""
    _dev(qkv)
    M, Wd = qkv.shape
    d = 32
    assert M == B * H * W and Wd == 3 * heads * d and qkv.stride(1) == 1
    if tuple(table.shape) != ((2 * window - 1) ** 2, heads):
        raise L.OmgHipError(f"attn_swin: the bias table is {tuple(table.shape)}, window {window} with {heads} heads needs "
                            f"({(2 * window - 1) ** 2}, {heads}) (no interpolation of the table)")
    assert table.is_contiguous() and table.dtype == qkv.dtype and table.is_cuda
    if pad_kv is not None:
        assert pad_kv.shape == (2 * heads * d,) and pad_kv.is_contiguous() and pad_kv.dtype == qkv.dtype and pad_kv.is_cuda
    if out is None:
        out = torch.empty((M, heads * d), dtype=qkv.dtype, device=qkv.device)
    assert out.shape[0] == M and out.shape[1] >= heads * d and out.stride(1) == 1 and out.dtype == qkv.dtype
    L.check(L.lib().omg_attn_swin(_dt(qkv), B, H, W, heads, window, shift, qkv.data_ptr(), qkv.stride(0), table.data_ptr(), _p(pad_kv),
                                  scale, out.data_ptr(), out.stride(0), _stream()), "omg_attn_swin")
    return out


def swin_patch_embed(x_nchw: torch.Tensor, dtype: torch.dtype, ld: int = 64, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NCHW pixel values [B, 3, H, W] (fp32 or ``dtype``) -> the 4x4 stride-4 patch rows [B*ceil(H/4)*ceil(W/4), ld] in ``dtype``:
    column k = (c*4 + ky)*4 + kx, zeros beyond the image and in columns 48 .. ld-1.  omg_swin_patch_embed."""
    _dev(x_nchw)
    B, Cin, H, W = x_nchw.shape
    assert Cin == 3 and x_nchw.is_contiguous() and x_nchw.dtype in (torch.float32, dtype)
    y = _out(out, (B * ((H + 3) // 4) * ((W + 3) // 4), ld), dtype, x_nchw.device)
    L.check(L.lib().omg_swin_patch_embed(_dt(x_nchw, allow_f32=True), _DT[dtype], x_nchw.data_ptr(), B, H, W, y.data_ptr(), ld, _stream()),
            "omg_swin_patch_embed")
    return y


def swin_merge_ln(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Patch merging's gather and LayerNorm: NHWC ``x`` [B, H, W, C] -> [B*ceil(H/2)*ceil(W/2), 4C], channel blocks (0,0), (1,0), (0,1),
    (1,1), an odd H or W zero-padded before the norm.  omg_swin_merge_ln."""
    _dev(x)
    B, H, W, Cc = x.shape
    assert x.is_contiguous() and gamma.shape == (4 * Cc,) and beta.shape == (4 * Cc,) and gamma.dtype == x.dtype and beta.dtype == x.dtype
    assert gamma.is_contiguous() and beta.is_contiguous()
    y = _out(out, (B * ((H + 1) // 2) * ((W + 1) // 2), 4 * Cc), x.dtype, x.device)
    L.check(L.lib().omg_swin_merge_ln(_dt(x), x.data_ptr(), B, H, W, Cc, gamma.data_ptr(), beta.data_ptr(), eps, y.data_ptr(), _stream()),
            "omg_swin_merge_ln")
    return y


def _bytes(m: Optional[torch.Tensor], shape, device) -> Optional[torch.Tensor]:
    """A [..] bool / uint8 mask (1 = valid / attend) as contiguous bytes on ``device``; None stays None."""
    if m is None:
        return None
    assert tuple(m.shape) == tuple(shape) and m.dtype in (torch.bool, torch.uint8) and m.device == device, (tuple(m.shape), m.dtype)
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def msdeform_attn(value: torch.Tensor, ow: torch.Tensor, ref: torch.Tensor, spatial_shapes: Sequence[Tuple[int, int]], *, heads: int = 8,
                  points: int = 4, mask: Optional[torch.Tensor] = None, level_start: Optional[Sequence[int]] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Multi-scale deformable attention between its Linear layers.  ``value`` [B, N, heads*32] (the rows of value_proj; a row stride that
    is a multiple of 8 is fine), ``ow`` [B, Nq, heads*L*12] = sampling_offsets | attention_weights of the queries, ``ref`` [B, Nq, L, 2]
    fp32 (x, y), ``spatial_shapes`` [(H_l, W_l)] with level l at rows ``level_start[l]`` (default: one after the other), ``mask`` [B, N]
    bool / uint8, 0 = the value row reads as zeros -> [B, Nq, heads*32].  omg_msdeform_attn."""
    return _msdeform(value, ow, ref, spatial_shapes, heads, points, mask, level_start, out, 2)


def msdeform_attn_box(value: torch.Tensor, ow: torch.Tensor, ref: torch.Tensor, spatial_shapes: Sequence[Tuple[int, int]], *, heads: int = 8,
                      points: int = 4, mask: Optional[torch.Tensor] = None, level_start: Optional[Sequence[int]] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`msdeform_attn` with box reference points ``ref`` [B, Nq, L, 4] fp32 (cx, cy, w, h) per sampled level (the decoder's
    ``reference_points_input``): a point's location is ``(cx, cy) + off / 4 * (w, h) * 0.5``.  omg_msdeform_attn_box."""
    return _msdeform(value, ow, ref, spatial_shapes, heads, points, mask, level_start, out, 4)


def _msdeform(value, ow, ref, spatial_shapes, heads, points, mask, level_start, out, coords):
    _dev(value)
    B, N, Wd = value.shape
    Nq = ow.shape[1]
    Lv = len(spatial_shapes)
    if not 1 <= Lv <= 4:
        raise L.OmgHipError(f"msdeform_attn: {Lv} levels; the kernel takes 1 to 4")
    assert Wd % heads == 0 and value.stride(2) == 1 and (B == 1 or value.stride(0) == N * value.stride(1))
    assert ow.shape == (B, Nq, heads * Lv * points * 3) and ow.stride(2) == 1 and (B == 1 or ow.stride(0) == Nq * ow.stride(1)) and ow.dtype == value.dtype
    assert ref.shape == (B, Nq, Lv, coords) and ref.dtype == torch.float32 and ref.is_contiguous() and ref.is_cuda
    mask = _bytes(mask, (B, N), value.device)
    if level_start is None:
        level_start, s = [], 0
        for (h_, w_) in spatial_shapes:
            level_start.append(s)
            s += int(h_) * int(w_)
    if out is None:
        out = torch.empty((B, Nq, Wd), dtype=value.dtype, device=value.device)
    assert out.shape[:2] == (B, Nq) and out.shape[2] >= Wd and out.stride(2) == 1 and out.dtype == value.dtype
    assert B == 1 or out.stride(0) == Nq * out.stride(1)
    a = L.MsdeformArgs()
    a.dtype, a.B, a.N, a.Nq, a.heads, a.head_dim, a.L, a.points = _dt(value), B, N, Nq, heads, Wd // heads, Lv, points
    for i, (h_, w_) in enumerate(spatial_shapes):
        a.H[i], a.W[i], a.start[i] = int(h_), int(w_), int(level_start[i])
    a.value, a.ldv, a.mask = value.data_ptr(), value.stride(1), _p(mask)
    a.ow, a.ldow, a.ref = ow.data_ptr(), ow.stride(1), ref.data_ptr()
    a.out, a.ldo = out.data_ptr(), out.stride(1)
    t0 = _PROF.begin() if _PROF is not None else None
    if coords == 4:
        L.check(L.lib().omg_msdeform_attn_box(C.byref(a), _stream()), "omg_msdeform_attn_box")
    else:
        L.check(L.lib().omg_msdeform_attn(C.byref(a), _stream()), "omg_msdeform_attn")
    if _PROF is not None:
        _PROF.end("msdeform_attn", 2.0 * B * Nq * Wd * Lv * points * 4, t0, ("msdeform_attn", Nq, N, Lv))
    return out


def _bi_operands(vis: torch.Tensor, txt: torch.Tensor, heads: int):
    _dev(vis)
    B, N, Wv = vis.shape
    T = txt.shape[1]
    assert Wv == 2 * heads * 256 and txt.shape == (B, T, Wv) and txt.dtype == vis.dtype and vis.stride(2) == 1 and txt.stride(2) == 1
    return B, N, T


def attn_bi_vision(vis: torch.Tensor, txt: torch.Tensor, heads: int, scale: float, *, text_mask: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The image side of GroundingDINO's bi-attention at head_dim 256: ``vis`` [B, N, 2*heads*256] = vision q | vision v, ``txt``
    [B, T <= 256, 2*heads*256] = text k | text v -> softmax over the text keys (``text_mask`` [B, T], 0 = padded) times the text values,
    [B, N, heads*256].  omg_attn_bi_vision."""
    B, N, T = _bi_operands(vis, txt, heads)
    text_mask = _bytes(text_mask, (B, T), vis.device)
    if out is None:
        out = torch.empty((B, N, heads * 256), dtype=vis.dtype, device=vis.device)
    assert out.shape == (B, N, heads * 256) and out.stride(2) == 1 and out.dtype == vis.dtype
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_attn_bi_vision(_dt(vis), B, heads, N, T, vis.data_ptr(), vis.stride(1), vis.stride(0), txt.data_ptr(), txt.stride(1),
                                       txt.stride(0), _p(text_mask), scale, out.data_ptr(), out.stride(1), out.stride(0), _stream()),
            "omg_attn_bi_vision")
    if _PROF is not None:
        _PROF.end("attn_bi_vision", 4.0 * B * heads * N * T * 256, t0, ("attn_bi_vision", N, T))
    return out


def attn_bi_text_chunk(N: int) -> int:
    """Image keys per workgroup of :func:`attn_bi_text`: a function of N alone.  omg_attn_bi_text_chunk."""
    return int(L.lib().omg_attn_bi_text_chunk(int(N)))


def attn_bi_text(vis: torch.Tensor, txt: torch.Tensor, heads: int, scale: float, *, vision_mask: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The text side of the bi-attention: softmax over all N image keys (``vision_mask`` [B, N], 0 = padded) times the vision values,
    [B, T, heads*256].  Operands as :func:`attn_bi_vision`; the chunk partials live in a workspace allocated per call (as
    :func:`groupnorm`'s).  omg_attn_bi_text."""
    B, N, T = _bi_operands(vis, txt, heads)
    vision_mask = _bytes(vision_mask, (B, N), vis.device)
    if out is None:
        out = torch.empty((B, T, heads * 256), dtype=vis.dtype, device=vis.device)
    assert out.shape == (B, T, heads * 256) and out.stride(2) == 1 and out.dtype == vis.dtype
    ws = torch.empty(max(int(L.lib().omg_attn_bi_text_ws_floats(B, heads, T, N)), 4), dtype=torch.float32, device=vis.device)
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_attn_bi_text(_dt(vis), B, heads, N, T, vis.data_ptr(), vis.stride(1), vis.stride(0), txt.data_ptr(), txt.stride(1),
                                     txt.stride(0), _p(vision_mask), scale, ws.data_ptr(), out.data_ptr(), out.stride(1), out.stride(0),
                                     _stream()), "omg_attn_bi_text")
    if _PROF is not None:
        _PROF.end("attn_bi_text", 4.0 * B * heads * N * T * 256, t0, ("attn_bi_text", N, T))
    return out


def attn_masked(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, *, mask: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``softmax(q k^T scale under mask) v`` per head at head_dim 64: ``q`` [B, Nq, heads*64], ``k`` / ``v`` [B, Nk, heads*64], Nq, Nk <= 256,
    ``mask`` [B, Nq, Nk] bool / uint8 (1 = attend, the same for every head) -> [B, Nq, heads*64].  Column slices of a projection buffer
    are fine.  omg_attn_masked."""
    _dev(q)
    B, Nq, Wd = q.shape
    Nk = k.shape[1]
    assert Wd == heads * 64 and k.shape == (B, Nk, Wd) and v.shape == (B, Nk, Wd) and k.dtype == q.dtype and v.dtype == q.dtype
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    mask = _bytes(mask, (B, Nq, Nk), q.device)
    if out is None:
        out = torch.empty((B, Nq, Wd), dtype=q.dtype, device=q.device)
    assert out.shape == (B, Nq, Wd) and out.stride(2) == 1 and out.dtype == q.dtype
    L.check(L.lib().omg_attn_masked(_dt(q), B, heads, Nq, Nk, q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0),
                                    v.data_ptr(), v.stride(1), v.stride(0), _p(mask), scale, out.data_ptr(), out.stride(1), out.stride(0),
                                    _stream()), "omg_attn_masked")
    return out


def attn_hd32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, *, key_mask: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``softmax(q k^T scale under key_mask) v`` per head at head_dim 32: ``q`` [B, Nq, heads*32], ``k`` / ``v`` [B, Nk, heads*32], any Nq,
    Nk >= 1, ``key_mask`` [B, Nk] bool / uint8 (1 = attend) -> [B, Nq, heads*32].  Column slices of a projection buffer are fine.
    omg_attn_hd32."""
    _dev(q)
    B, Nq, Wd = q.shape
    Nk = k.shape[1]
    assert Wd == heads * 32 and k.shape == (B, Nk, Wd) and v.shape == (B, Nk, Wd) and k.dtype == q.dtype and v.dtype == q.dtype
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    key_mask = _bytes(key_mask, (B, Nk), q.device)
    if out is None:
        out = torch.empty((B, Nq, Wd), dtype=q.dtype, device=q.device)
    assert out.shape == (B, Nq, Wd) and out.stride(2) == 1 and out.dtype == q.dtype
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_attn_hd32(_dt(q), B, heads, Nq, Nk, q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0),
                                  v.data_ptr(), v.stride(1), v.stride(0), _p(key_mask), scale, out.data_ptr(), out.stride(1), out.stride(0),
                                  _stream()), "omg_attn_hd32")
    if _PROF is not None:
        _PROF.end("attn_hd32", 4.0 * B * Nq * Nk * Wd, t0, ("attn_hd32", Nq, Nk))
    return out


def gdino_contrastive(x: torch.Tensor, y: torch.Tensor, text_mask: torch.Tensor, max_text_len: int = 256, *, logits: bool = True,
                      rowmax: bool = False):
    """GroundingDinoContrastiveEmbedding: ``x`` [B, N, 256], ``y`` [B, T, 256] (row strides multiples of 8), ``text_mask`` [B, T] bool /
    uint8 -> the fp32 logits [B, N, max_text_len] (-inf on masked tokens and beyond T), their row maximum [B, N], or (logits, rowmax) —
    whichever of the two is asked for; with ``logits=False`` no [B, N, T] tensor is written.  omg_gdino_contrastive."""
    _dev(x)
    B, N, Wd = x.shape
    T = y.shape[1]
    assert Wd == 256 and y.shape == (B, T, 256) and y.dtype == x.dtype and x.stride(2) == 1 and y.stride(2) == 1
    assert (B == 1 or x.stride(0) == N * x.stride(1)) and (B == 1 or y.stride(0) == T * y.stride(1))
    assert logits or rowmax
    text_mask = _bytes(text_mask, (B, T), x.device)
    lg = torch.empty((B, N, max_text_len), dtype=torch.float32, device=x.device) if logits else None
    rm = torch.empty((B, N), dtype=torch.float32, device=x.device) if rowmax else None
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_gdino_contrastive(_dt(x), B, N, T, int(max_text_len), x.data_ptr(), x.stride(1), y.data_ptr(), y.stride(1),
                                          _p(text_mask), _p(lg), _p(rm), _stream()), "omg_gdino_contrastive")
    if _PROF is not None:
        _PROF.end("gdino_contrastive", 2.0 * B * N * T * 256, t0, ("gdino_contrastive", N, T))
    return (lg, rm) if logits and rowmax else (lg if logits else rm)


def gdino_ref_step(valid_ratios: torch.Tensor, *, ref_in: Optional[torch.Tensor] = None, logit_in: Optional[torch.Tensor] = None,
                   hidden: Optional[torch.Tensor] = None, w3: Optional[torch.Tensor] = None, b3: Optional[torch.Tensor] = None,
                   dtype: Optional[torch.dtype] = None, embed: bool = True):
    """One decoder layer's reference bookkeeping.  ``ref_in`` [B, Q, 4] fp32 (its ``torch.special.logit(eps=1e-5)`` is the base) or
    ``logit_in`` [B, Q, 4] fp32 (the base itself, +inf allowed); ``hidden`` [B, Q, 256] (the box head's second hidden state, 16-bit) with
    the head's last Linear ``w3`` [4, 256], ``b3`` [4], or None (``ref_out = ref_in`` / ``sigmoid(logit_in)``); ``valid_ratios`` [B, L, 2]
    fp32 -> (ref_out [B, Q, 4], ref_input [B, Q, L, 4], embedding [B, Q, 512] in the storage type or None).  omg_gdino_ref_step."""
    base = ref_in if ref_in is not None else logit_in
    assert base is not None and (ref_in is None or logit_in is None)
    _dev(base)
    B, Q, _ = base.shape
    Lv = valid_ratios.shape[1]
    assert base.shape == (B, Q, 4) and base.dtype == torch.float32 and base.is_contiguous()
    assert valid_ratios.shape == (B, Lv, 2) and valid_ratios.dtype == torch.float32 and valid_ratios.is_contiguous() and valid_ratios.is_cuda
    if hidden is not None:
        assert hidden.shape == (B, Q, 256) and hidden.stride(2) == 1 and (B == 1 or hidden.stride(0) == Q * hidden.stride(1))
        assert w3.shape == (4, 256) and b3.shape == (4,) and w3.dtype == hidden.dtype and b3.dtype == hidden.dtype and w3.is_contiguous()
        dtype = hidden.dtype
    assert dtype in (torch.float16, torch.bfloat16)
    ref_out = torch.empty((B, Q, 4), dtype=torch.float32, device=base.device)
    ref_input = torch.empty((B, Q, Lv, 4), dtype=torch.float32, device=base.device)
    emb = torch.empty((B, Q, 512), dtype=dtype, device=base.device) if embed else None
    L.check(L.lib().omg_gdino_ref_step(L.OMG_F16 if dtype == torch.float16 else L.OMG_BF16, B, Q, Lv, _p(ref_in), _p(logit_in),
                                       valid_ratios.data_ptr(), _p(hidden), hidden.stride(1) if hidden is not None else 0, _p(w3), _p(b3),
                                       ref_out.data_ptr(), ref_input.data_ptr(), _p(emb), 512, _stream()), "omg_gdino_ref_step")
    return ref_out, ref_input, emb


def gemm_skinny(a: torch.Tensor, w: torch.Tensor, *, bias: Optional[torch.Tensor] = None, gelu: bool = False,
                residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[M, N] = epi(a[M, K] @ w[N, K]^T)`` for few rows: bias, then the erf GELU, then the residual.  Rows may be column slices of
    wider buffers (unit column stride).  omg_gemm_skinny."""
    _dev(a)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and a.stride(1) == 1 and w.stride(1) == 1 and w.dtype == a.dtype
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == a.dtype
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1 and residual.dtype == a.dtype
    if bias is not None:
        assert bias.shape == (N,) and bias.is_contiguous() and bias.dtype == a.dtype and bias.device == a.device
    assert w.device == a.device and out.device == a.device and (residual is None or residual.device == a.device)
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_gemm_skinny(_dt(a), M, N, K, a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias), int(gelu),
                                    _p(residual), residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0),
                                    _stream()), "omg_gemm_skinny")
    if _PROF is not None:
        _PROF.end("gemm_skinny", 2.0 * M * N * K, t0, ("skinny", M, N, K))
    return out


def bert_embed_ln(input_ids: torch.Tensor, token_type_ids: torch.Tensor, position_ids: torch.Tensor, word: torch.Tensor,
                  token_type: torch.Tensor, position: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``LayerNorm(word[input_ids] + token_type[token_type_ids] + position[position_ids])``: the ids int64 of one shape [...], the tables
    [rows, C] contiguous -> [..., C].  An id outside its table is clamped into it.  omg_bert_embed_ln."""
    _dev(word)
    C_ = word.shape[1]
    for t in (input_ids, token_type_ids, position_ids):
        if t.dtype != torch.int64 or t.shape != input_ids.shape or not t.is_contiguous() or t.device != word.device:
            raise L.OmgHipError("bert_embed_ln: the ids are contiguous int64 tensors of one shape on the tables' device")
    for t in (word, token_type, position):
        assert t.dim() == 2 and t.shape[1] == C_ and t.is_contiguous() and t.dtype == word.dtype and t.device == word.device
    for t in (gamma, beta):
        assert t.shape == (C_,) and t.is_contiguous() and t.dtype == word.dtype and t.device == word.device
    M = input_ids.numel()
    if out is None:
        out = torch.empty(tuple(input_ids.shape) + (C_,), dtype=word.dtype, device=word.device)
    assert out.is_contiguous() and out.numel() == M * C_ and out.dtype == word.dtype
    L.check(L.lib().omg_bert_embed_ln(_dt(word), M, C_, input_ids.data_ptr(), token_type_ids.data_ptr(), position_ids.data_ptr(),
                                      word.data_ptr(), word.shape[0], token_type.data_ptr(), token_type.shape[0], position.data_ptr(),
                                      position.shape[0], gamma.data_ptr(), beta.data_ptr(), eps, out.data_ptr(), C_, _stream()),
            "omg_bert_embed_ln")
    return out


def conv3x3_nhwc_ex(x: torch.Tensor, w: torch.Tensor, *, stride: int = 1, bias: Optional[torch.Tensor] = None, act: int = 0,
                    residual: Optional[torch.Tensor] = None, relu_in: bool = False, same: bool = False,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`conv3x3_nhwc_act`'s kernel with ``act`` 0 | 1 (tanh GELU) | 2 (ReLU), ReLU of the input as it is loaded (``relu_in``; the
    residual is read as stored) and, at stride 2, TF-"SAME" padding (``same``: nothing in front of an even size).  omg_conv3x3_nhwc_ex."""
    _dev(x)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and w.shape == (Cout, 3, 3, Cin) and w.dtype == x.dtype
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    assert out.shape == (B, Ho, Wo, Cout) and out.is_contiguous() and out.dtype == x.dtype
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous() and residual.dtype == x.dtype
    t0 = _PROF.begin() if _PROF is not None else None
    L.check(L.lib().omg_conv3x3_nhwc_ex(_dt(x), x.data_ptr(), B, H, W, Cin, Cout, stride, w.data_ptr(), _p(bias), int(act), _p(residual),
                                        int(relu_in) | (int(same) << 1), out.data_ptr(), _stream()), "omg_conv3x3_nhwc_ex")
    if _PROF is not None:
        _PROF.end("conv3x3_nhwc", 2.0 * B * Ho * Wo * Cout * 9 * Cin, t0, ("conv3x3_nhwc", B * Ho * Wo, Cout, 9 * Cin, stride))
    return out


def _out(out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    assert tuple(out.shape) == tuple(shape) and out.is_contiguous() and out.dtype == dtype and out.device == device
    return out


def pack_dpt_stem_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """[Cout, 3, 7, 7] -> [Cout, 148]: k = (ky * 7 + kx) * 3 + c, one zero behind (74 pairs for the packed dot products)."""
    cout = w_oihw.shape[0]
    assert w_oihw.shape[1:] == (3, 7, 7)
    out = torch.zeros((cout, 148), dtype=w_oihw.dtype, device=w_oihw.device)
    out[:, :147] = w_oihw.permute(0, 2, 3, 1).reshape(cout, 147)
    return out


def dpt_stem_conv(x_nchw: torch.Tensor, w_packed: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BiT's stem: 7x7 stride-2 convolution, TF-"SAME" padding, of NCHW pixel values (fp32 or the weights' dtype) -> NHWC
    [B, ceil(H/2), ceil(W/2), Cout] in the weights' dtype.  ``w_packed`` from :func:`pack_dpt_stem_weight`.  omg_dpt_stem_conv."""
    _dev(x_nchw)
    B, Cin, H, W = x_nchw.shape
    Cout = w_packed.shape[0]
    assert Cin == 3 and x_nchw.is_contiguous() and w_packed.shape == (Cout, 148) and w_packed.is_contiguous()
    assert x_nchw.dtype in (torch.float32, w_packed.dtype)
    y = _out(out, (B, (H + 1) // 2, (W + 1) // 2, Cout), w_packed.dtype, x_nchw.device)
    L.check(L.lib().omg_dpt_stem_conv(_dt(x_nchw, allow_f32=True), _dt(w_packed), x_nchw.data_ptr(), B, H, W, Cout, w_packed.data_ptr(),
                                      y.data_ptr(), _stream()), "omg_dpt_stem_conv")
    return y


def groupnorm_res_act(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, *,
                      residual: Optional[torch.Tensor] = None, relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``relu?(GroupNorm(x) * gamma + beta [+ residual])`` of NHWC ``x`` (B, H, W, C) or (B, HW, C): :func:`groupnorm`'s statistics,
    the residual add and the ReLU in the apply pass.  omg_groupnorm_res_act."""
    _dev(x)
    assert x.is_contiguous() and gamma.dtype == x.dtype and beta.dtype == x.dtype
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // max(B * Cc, 1)
    if residual is not None:
        assert residual.shape == x.shape and residual.is_contiguous() and residual.dtype == x.dtype
    y = _out(out, tuple(x.shape), x.dtype, x.device)
    ws = _gn_workspace(x.device, B, groups, HW)
    L.check(L.lib().omg_groupnorm_res_act(_dt(x), x.data_ptr(), B, HW, Cc, groups, eps, gamma.data_ptr(), beta.data_ptr(), _p(residual),
                                          int(relu), ws.data_ptr(), y.data_ptr(), _stream()), "omg_groupnorm_res_act")
    return y


def maxpool3x3s2_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 stride-2 max-pool of NHWC ``x`` under TF-"SAME" padding with pad value 0 -> [B, ceil(H/2), ceil(W/2), C].  omg_maxpool3x3s2_nhwc."""
    _dev(x)
    B, H, W, Cc = x.shape
    assert x.is_contiguous()
    y = _out(out, (B, (H + 1) // 2, (W + 1) // 2, Cc), x.dtype, x.device)
    L.check(L.lib().omg_maxpool3x3s2_nhwc(_dt(x), x.data_ptr(), B, H, W, Cc, y.data_ptr(), _stream()), "omg_maxpool3x3s2_nhwc")
    return y


def upsample2x_bilinear_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Bilinear x2 resize (align_corners=True) of NHWC ``x`` -> [B, 2H, 2W, C].  omg_upsample2x_bilinear_nhwc."""
    _dev(x)
    B, H, W, Cc = x.shape
    assert x.is_contiguous()
    y = _out(out, (B, 2 * H, 2 * W, Cc), x.dtype, x.device)
    L.check(L.lib().omg_upsample2x_bilinear_nhwc(_dt(x), x.data_ptr(), B, H, W, Cc, y.data_ptr(), _stream()), "omg_upsample2x_bilinear_nhwc")
    return y


def rowdot_f32(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``relu?(x @ w + bias)`` in fp32 for rows ``x`` [M, C] (unit inner stride), ``w`` [C], ``bias`` [1] -> fp32 [M].  omg_rowdot_f32."""
    _dev(x)
    M, Cc = x.shape
    assert x.stride(1) == 1 and w.shape == (Cc,) and w.is_contiguous() and w.dtype == x.dtype
    if bias is not None:
        assert bias.numel() == 1 and bias.dtype == x.dtype
    y = _out(out, (M,), torch.float32, x.device)
    L.check(L.lib().omg_rowdot_f32(_dt(x), x.data_ptr(), x.stride(0), M, Cc, w.data_ptr(), _p(bias), int(relu), y.data_ptr(), _stream()), "omg_rowdot_f32")
    return y


def depth_tail(depth: torch.Tensor, size: Tuple[int, int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The tail of the demos' ``get_depth``: fp32 ``depth`` [B, h, w] -> uint8 [B, H, W, 3]: bicubic resize (align_corners=False) to
    ``size``, min-max normalisation of the resized map per sample, x 255, clipped and truncated, three equal channels.  A constant map
    gives zeros.  omg_depth_tail."""
    _dev(depth)
    if depth.dtype != torch.float32 or depth.dim() != 3:
        raise L.OmgHipError(f"depth_tail takes a float32 [B, h, w] map, not {depth.dtype} {tuple(depth.shape)}")
    B, h, w = depth.shape
    H, W = int(size[0]), int(size[1])
    assert depth.is_contiguous()
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=depth.device)
    assert out.shape == (B, H, W, 3) and out.is_contiguous() and out.dtype == torch.uint8
    ws = torch.empty((max(int(L.lib().omg_depth_tail_ws_floats(B, H, W)), 1),), dtype=torch.float32, device=depth.device)      # per call: see _gn_workspace
    L.check(L.lib().omg_depth_tail(depth.data_ptr(), B, h, w, H, W, ws.data_ptr(), out.data_ptr(), _stream()), "omg_depth_tail")
    return out


def conv_in(x_nchw: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """NCHW latents (fp32 or `dtype`) -> NHWC features in `dtype`; w: [Cout][64] from pack_conv_in_weight."""
    _dev(x_nchw)
    assert x_nchw.is_contiguous()
    B, Cin, H, W = x_nchw.shape
    Cout = w.shape[0]
    assert w.shape[1] == 64 and w.is_contiguous()
    y = torch.empty((B, H, W, Cout), dtype=dtype, device=x_nchw.device)
    ws = torch.empty((B * H * W, 64), dtype=dtype, device=x_nchw.device)
    is_f32 = x_nchw.dtype == torch.float32
    assert is_f32 or x_nchw.dtype == dtype
    L.check(L.lib().omg_conv_in(_DT[dtype], x_nchw.data_ptr(), int(is_f32), B, Cin, H, W, w.data_ptr(), _p(bias), Cout,
                                ws.data_ptr(), y.data_ptr(), _stream()), "omg_conv_in")
    return y


def conv_out(x_nhwc: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor],
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NHWC features -> NCHW fp32; w: [Cout][3][3][Cin]."""
    _dev(x_nhwc)
    assert x_nhwc.is_contiguous()
    B, H, W, Cin = x_nhwc.shape
    Cout = w.shape[0]
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x_nhwc.device)
    assert out.is_contiguous() and out.dtype == torch.float32
    assert w.dtype == x_nhwc.dtype and (bias is None or bias.dtype == x_nhwc.dtype)
    L.check(L.lib().omg_conv_out(_dt(x_nhwc, allow_f32=True), x_nhwc.data_ptr(), B, H, W, Cin, w.data_ptr(), _p(bias), Cout,
                                 out.data_ptr(), _stream()), "omg_conv_out")
    return out


def softmax_rows_(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """In-place ``softmax(x * scale, dim=-1)`` of a 2-D tensor with unit inner stride (VAE mid-block attention scores)."""
    _dev(x)
    assert x.dim() == 2 and x.stride(1) == 1
    L.check(L.lib().omg_softmax_rows(_dt(x), x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), float(scale), _stream()),
            "omg_softmax_rows")
    return x


def channel_mix(x_nchw: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """fp32 NCHW 1x1 convolution with at most 8 channels on either side (AutoencoderKL.post_quant_conv)."""
    _dev(x_nchw)
    assert x_nchw.dtype == torch.float32 and x_nchw.is_contiguous() and w.dtype == torch.float32 and w.is_contiguous()
    B, Cin, H, W = x_nchw.shape
    Cout = w.shape[0]
    assert w.numel() == Cout * Cin and (bias is None or (bias.dtype == torch.float32 and bias.numel() == Cout))
    y = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x_nchw.device)
    L.check(L.lib().omg_channel_mix(x_nchw.data_ptr(), w.data_ptr(), _p(bias), B, Cin, Cout, H * W, y.data_ptr(), _stream()),
            "omg_channel_mix")
    return y


def timestep_embedding(t: torch.Tensor, dim: int, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """t: fp32 device tensor [n] -> [n, dim] (cos | sin), written into `out` (may be a column slice)."""
    _dev(t)
    assert t.dtype == torch.float32 and t.is_contiguous()
    n = t.numel()
    if out is None:
        out = torch.empty((n, dim), dtype=dtype, device=t.device)
    assert out.stride(1) == 1
    L.check(L.lib().omg_timestep_embedding(_DT[dtype], t.data_ptr(), n, dim, out.data_ptr(), out.stride(0), _stream()),
            "omg_timestep_embedding")
    return out


def silu(x: torch.Tensor) -> torch.Tensor:
    _dev(x)
    assert x.is_contiguous()
    y = torch.empty_like(x)
    L.check(L.lib().omg_silu(_dt(x), x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "omg_silu")
    return y


def add_(y: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """y += a (same shape, contiguous)."""
    _dev(y)
    assert y.is_contiguous() and a.is_contiguous() and y.shape == a.shape and y.dtype == a.dtype
    L.check(L.lib().omg_add_inplace(_dt(y), y.data_ptr(), a.data_ptr(), y.numel(), _stream()), "omg_add_inplace")
    return y


def copy2d(src: torch.Tensor, dst: torch.Tensor) -> None:
    """dst[r, :cols] = src[r, :cols] for 2-D views with unit inner stride."""
    _dev(src)
    assert src.dim() == 2 and dst.dim() == 2 and src.shape == dst.shape and src.stride(1) == 1 and dst.stride(1) == 1
    L.check(L.lib().omg_copy2d(_dt(src), src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), src.shape[0],
                               src.shape[1], _stream()), "omg_copy2d")


def _step_args(noise_pred: torch.Tensor, latents: torch.Tensor, step_idx: torch.Tensor, guidance_scale: float, fuse: bool,
               region_preds: Sequence[Optional[torch.Tensor]], masks: Sequence[Optional[torch.Tensor]],
               model_input_next: Optional[torch.Tensor], advance: bool, fused_noise_out: Optional[torch.Tensor]) -> L.StepArgs:
    """omg_step_args of both step entry points, without the scheduler table"""
    _dev(noise_pred)
    assert noise_pred.dtype == torch.float32 and noise_pred.is_contiguous() and noise_pred.shape[0] == 4
    assert latents.dtype == torch.float32 and latents.is_contiguous() and latents.shape[0] == 2
    assert step_idx.dtype == torch.int32
    _, Cc, H, W = noise_pred.shape
    a = L.StepArgs()
    a.C, a.H, a.W = Cc, H, W
    a.n_concepts = len(masks)
    assert len(region_preds) == len(masks) <= L.MAX_CONCEPTS
    a.fuse = int(fuse)
    a.guidance_scale = guidance_scale
    a.noise_pred = noise_pred.data_ptr()
    hm = wm = 0
    for i, (r, m) in enumerate(zip(region_preds, masks)):
        if r is not None:
            assert r.dtype == torch.float32 and r.is_contiguous() and r.shape == (2, Cc, H, W)
            a.region_pred[i] = r.data_ptr()
        if m is not None:
            assert m.dtype == torch.float32 and m.is_contiguous() and m.dim() == 2
            if hm:
                assert (hm, wm) == tuple(m.shape), "all masks must share one resolution"
            hm, wm = m.shape
            a.masks[i] = m.data_ptr()
    a.Hm, a.Wm = (hm, wm) if hm else (H, W)
    a.step_idx, a.advance = step_idx.data_ptr(), int(advance)
    a.latents = latents.data_ptr()
    if model_input_next is not None:
        assert model_input_next.is_contiguous() and model_input_next.shape == (4, Cc, H, W)
        a.model_input_next = model_input_next.data_ptr()
        a.out_dtype = L.OMG_F32 if model_input_next.dtype == torch.float32 else _dt(model_input_next)
    if fused_noise_out is not None:
        assert fused_noise_out.dtype == torch.float32 and fused_noise_out.is_contiguous()
        a.fused_noise_out = fused_noise_out.data_ptr()
    return a


def fuse_cfg_step(noise_pred: torch.Tensor, latents: torch.Tensor, coef: torch.Tensor, step_idx: torch.Tensor, *,
                  guidance_scale: float, fuse: bool = False, region_preds: Sequence[Optional[torch.Tensor]] = (),
                  masks: Sequence[Optional[torch.Tensor]] = (), model_input_next: Optional[torch.Tensor] = None,
                  advance: bool = True, fused_noise_out: Optional[torch.Tensor] = None) -> None:
    """Region fusion + CFG + scheduler step + next model input (see omg_fuse_cfg_step)."""
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.shape[-1] == 4
    a = _step_args(noise_pred, latents, step_idx, guidance_scale, fuse, region_preds, masks, model_input_next, advance, fused_noise_out)
    a.coef = coef.data_ptr()
    L.check(L.lib().omg_fuse_cfg_step(C.byref(a), _stream()), "omg_fuse_cfg_step")


def fuse_cfg_step_ms(noise_pred: torch.Tensor, latents: torch.Tensor, ms_coef: torch.Tensor, x0_hist: torch.Tensor, step_idx: torch.Tensor, *,
                     guidance_scale: float, fuse: bool = False, region_preds: Sequence[Optional[torch.Tensor]] = (),
                     masks: Sequence[Optional[torch.Tensor]] = (), model_input_next: Optional[torch.Tensor] = None,
                     advance: bool = True, fused_noise_out: Optional[torch.Tensor] = None) -> None:
    """:func:`fuse_cfg_step` with a multistep scheduler update (see omg_fuse_cfg_step_ms): ``ms_coef`` (n, 8) fp32 from
    ``DPMSolverMultistepScheduler.coef_table``; ``x0_hist`` fp32 (2, C, H, W) holds the previous step's data prediction of both samples
    and receives this step's."""
    assert ms_coef.dtype == torch.float32 and ms_coef.is_contiguous() and ms_coef.dim() == 2 and ms_coef.shape[-1] == 8
    assert x0_hist.dtype == torch.float32 and x0_hist.is_contiguous() and x0_hist.shape == latents.shape and x0_hist.device == latents.device
    a = _step_args(noise_pred, latents, step_idx, guidance_scale, fuse, region_preds, masks, model_input_next, advance, fused_noise_out)
    L.check(L.lib().omg_fuse_cfg_step_ms(C.byref(a), ms_coef.data_ptr(), x0_hist.data_ptr(), _stream()), "omg_fuse_cfg_step_ms")


def fuse_cfg_step_noise(noise_pred: torch.Tensor, latents: torch.Tensor, coef: torch.Tensor, z: torch.Tensor, step_idx: torch.Tensor, *,
                        guidance_scale: float, fuse: bool = False, region_preds: Sequence[Optional[torch.Tensor]] = (),
                        masks: Sequence[Optional[torch.Tensor]] = (), model_input_next: Optional[torch.Tensor] = None,
                        advance: bool = True, fused_noise_out: Optional[torch.Tensor] = None) -> None:
    """:func:`fuse_cfg_step` with a stochastic scheduler update (see omg_fuse_cfg_step_noise): ``coef`` (n, 4) fp32 whose column 3 is
    the noise coefficient; ``z`` fp32 (n, 2, C, H, W), one noise draw per step (the step dimension may be strided, each step's block
    contiguous), selected on the device by ``step_idx``."""
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.dim() == 2 and coef.shape[-1] == 4
    assert z.dtype == torch.float32 and z.dim() == 5 and z.shape[0] == coef.shape[0] and z.shape[1:] == latents.shape and z.device == latents.device
    assert z[0].is_contiguous() and z.stride(0) >= z[0].numel()
    a = _step_args(noise_pred, latents, step_idx, guidance_scale, fuse, region_preds, masks, model_input_next, advance, fused_noise_out)
    a.coef = coef.data_ptr()
    L.check(L.lib().omg_fuse_cfg_step_noise(C.byref(a), z.data_ptr(), z.stride(0), _stream()), "omg_fuse_cfg_step_noise")


def gather_step(table: torch.Tensor, step_idx: torch.Tensor, out: torch.Tensor) -> None:
    """out = table[step_idx] with the step index read ON THE DEVICE (table: (S, ...), out: (...))."""
    _dev(table)
    assert table.is_contiguous() and out.is_contiguous() and table.shape[1:] == out.shape and step_idx.dtype == torch.int32
    L.check(L.lib().omg_gather_step(_dt(table), table.data_ptr(), step_idx.data_ptr(), out.data_ptr(), out.numel(), _stream()),
            "omg_gather_step")


def scale_model_input(latents: torch.Tensor, coef_cin: torch.Tensor, out: torch.Tensor) -> None:
    """out[4,C,H,W] = cin * cat([latents]*2); coef_cin: 1-element fp32 device tensor."""
    _dev(latents)
    assert latents.dtype == torch.float32 and latents.is_contiguous() and out.is_contiguous()
    n = latents[0].numel()
    dt = L.OMG_F32 if out.dtype == torch.float32 else _dt(out)
    L.check(L.lib().omg_scale_model_input(dt, latents.data_ptr(), coef_cin.data_ptr(), n, out.data_ptr(), _stream()),
            "omg_scale_model_input")


# ------------------------------------------------------------------ host-side weight packing
def pack_conv_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """diffusers conv weight [Cout, Cin, kh, kw] -> [Cout, kh*kw*Cin] (K = (tap, cin)); pure layout."""
    co, ci, kh, kw = w_oihw.shape
    return w_oihw.permute(0, 2, 3, 1).reshape(co, kh * kw * ci).contiguous()


def pack_conv_weight_phase(w_oihw: torch.Tensor) -> torch.Tensor:
    """3x3 conv weight [..., Cout, Cin, 3, 3] -> the phase image [..., 4, Cout, 4 * Cin] of the nearest-2x upsample + conv (``conv2d(upsample=2)``).

    Output pixel (2y + py, 2x + px) of the upsampled convolution reads the source rows y - 1 + py + a, a = 0, 1: for py = 0 row y - 1 with
    w[0] and row y with w[1] + w[2]; for py = 1 row y with w[0] + w[1] and row y + 1 with w[2] — the same along x.  Phase 2 py + px is the 2x2
    convolution with tap origin (py - 1, px - 1) whose taps (a, c), row-major, are those sums of 1, 2, 2 or 4 original taps; K = (tap, cin).
    Summed in fp32 (float64 for a float64 weight), rounded to the storage type once.  Any device; leading dimensions (weight slots) pass through."""
    assert w_oihw.dim() >= 4 and tuple(w_oihw.shape[-2:]) == (3, 3)
    lead, (co, ci) = tuple(w_oihw.shape[:-4]), w_oihw.shape[-4:-2]
    wf = w_oihw if w_oihw.dtype == torch.float64 else w_oihw.float()
    rows = ((wf[..., 0, :], wf[..., 1, :] + wf[..., 2, :]), (wf[..., 0, :] + wf[..., 1, :], wf[..., 2, :]))      # [py][a]: [..., Cout, Cin, 3]
    phases = []
    for py in range(2):
        for px in range(2):
            taps = []
            for a in range(2):
                r = rows[py][a]
                taps += [r[..., 0], r[..., 1] + r[..., 2]] if px == 0 else [r[..., 0] + r[..., 1], r[..., 2]]
            phases.append(torch.stack(taps, dim=-2))                 # [..., Cout, 4 taps, Cin]
    return torch.stack(phases, dim=-4).reshape(*lead, 4, co, 4 * ci).to(w_oihw.dtype).contiguous()


def pack_conv_weight_wino(w_oihw: torch.Tensor) -> torch.Tensor:
    """fp32 conv weight [Cout, Cin, 3, 3] -> the Winograd F(2x2, 3x3) image U = G g G^T that omg_conv2d_f32_wino streams:
    [ceil(Cout / 64)][Cin / 8][pos 16][k chunk 2][row 64][4], zero rows beyond Cout.  Built once per weight."""
    co, ci, kh, kw = w_oihw.shape
    assert kh == 3 and kw == 3 and ci % 8 == 0 and w_oihw.dtype == torch.float32
    def g_rows(t, dim):                                            # G t along ``dim``: [t0, (t0 + t1 + t2) / 2, (t0 - t1 + t2) / 2, t2]
        t0, t1, t2 = t.unbind(dim)
        return torch.stack((t0, (t0 + t1 + t2) * 0.5, (t0 - t1 + t2) * 0.5, t2), dim)
    # in float64, rounded to fp32 once: a sum of up to nine fp32 taps is exact to 2^-53 there, so every U is within half an ulp of its own
    # value.  Formed in fp32, a U whose taps cancel (a zero-sum filter's middle positions) carried an error relative to the taps instead,
    # which the large V of the same positions (sums of four pixels) multiplied up
    u = g_rows(g_rows(w_oihw.double(), 2), 3).float()              # [Cout, Cin, 4, 4]
    nb = (co + 63) // 64
    up = torch.zeros((nb * 64, ci, 4, 4), dtype=torch.float32, device=w_oihw.device)
    up[:co] = u
    up = up.view(nb, 64, ci // 8, 2, 4, 16)                         # [nb][row][stage][chunk][e][pos]
    return up.permute(0, 2, 5, 3, 1, 4).contiguous().view(-1)


def pack_conv_in_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """conv_in weight [Cout, Cin, 3, 3] -> [Cout, 64]: (ky, kx, ci) order, zero padded (one GEMM K-slice)."""
    co, ci, kh, kw = w_oihw.shape
    out = torch.zeros((co, 64), dtype=w_oihw.dtype, device=w_oihw.device)
    out[:, : kh * kw * ci] = w_oihw.permute(0, 2, 3, 1).reshape(co, kh * kw * ci)
    return out


def geglu_row_perm(n_total: int) -> torch.Tensor:
    """Row permutation that interleaves GEGLU value/gate rows in blocks of 32 (see gemm.hip epilogue).

    packed row p: block = p // 64, j = p % 64; j < 32 -> value row block*32 + j,
    else gate row n_total/2 + block*32 + (j - 32).
    """
    nh = n_total // 2
    assert nh % 32 == 0
    p = torch.arange(n_total)
    blk, j = p // 64, p % 64
    return torch.where(j < 32, blk * 32 + j, nh + blk * 32 + (j - 32))


_LUT_DT = {torch.float16: L.OMG_F16, torch.bfloat16: L.OMG_BF16, torch.float32: L.OMG_F32}


def image_prep(u8: torch.Tensor, out_hw: Tuple[int, int], resample: int, lut: Optional[torch.Tensor] = None,
               pad_hw: Optional[Tuple[int, int]] = None, out_dtype: Optional[torch.dtype] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``PIL.Image.resize((ow, oh), resample)`` of a contiguous cuda uint8 ``[H, W, 3]`` / ``[B, H, W, 3]`` image, bit for bit
    (``resample`` 2 BILINEAR or 3 BICUBIC; omg_amd/image_prep.py has the arithmetic).  Without ``lut``: the resized uint8 image
    ``[(B,) oh, ow, 3]``.  With ``lut`` ``[3, 256]`` of ``out_dtype`` (float16 / bfloat16 / float32): ``[(B,) 3, Hpad, Wpad]`` of that
    dtype, ``out[c, y, x] = lut[c, resized[y, x, c]]`` and zeros in the pad at the right and bottom (``pad_hw``, default none).  Two
    launches (omg_image_resize_h, omg_image_resize_v), one when an axis keeps its size; nothing else runs.  ``out``: the result's buffer."""
    from . import image_prep as ip
    if not isinstance(u8, torch.Tensor):
        raise L.OmgHipError(f"image_prep takes a contiguous cuda uint8 [H, W, 3] or [B, H, W, 3] tensor, got {type(u8).__name__}")
    if not u8.is_cuda or u8.dtype != torch.uint8 or u8.dim() not in (3, 4) or u8.shape[-1] != 3 or not u8.is_contiguous() or u8.numel() == 0:
        raise L.OmgHipError(f"image_prep takes a contiguous cuda uint8 [H, W, 3] or [B, H, W, 3] tensor, got {u8.dtype} {tuple(u8.shape)} "
                            f"on {u8.device}{'' if u8.is_contiguous() else ', not contiguous'}")
    try:
        resample = ip.check_resample(resample)
    except ValueError as e:
        raise L.OmgHipError(str(e)) from None
    batched = u8.dim() == 4
    B = u8.shape[0] if batched else 1
    H, W = int(u8.shape[-3]), int(u8.shape[-2])
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if oh < 1 or ow < 1:
        raise L.OmgHipError(f"image_prep: out_hw {tuple(out_hw)}")
    dev = u8.device
    if lut is None:
        if pad_hw is not None or out_dtype not in (None, torch.uint8):
            raise L.OmgHipError("image_prep: pad_hw and out_dtype go with a lookup table (the planar output); without one the result is uint8 HWC")
        code, hp, wp = 0, oh, ow
        shape, dt_out = (B, oh, ow, 3), torch.uint8
    else:
        out_dtype = lut.dtype if out_dtype is None else out_dtype
        if out_dtype not in _LUT_DT or lut.dtype != out_dtype or tuple(lut.shape) != (3, 256) or not lut.is_contiguous() or lut.device != dev:
            raise L.OmgHipError(f"image_prep: the lookup table is a contiguous [3, 256] tensor of out_dtype (float16, bfloat16 or float32) on the "
                                f"image's device, got {lut.dtype} {tuple(lut.shape)} on {lut.device} for out_dtype {out_dtype}")
        hp, wp = (oh, ow) if pad_hw is None else (int(pad_hw[0]), int(pad_hw[1]))
        if hp < oh or wp < ow:
            raise L.OmgHipError(f"image_prep: pad_hw {(hp, wp)} is smaller than out_hw {(oh, ow)}")
        code = _LUT_DT[out_dtype]
        shape, dt_out = (B, 3, hp, wp), out_dtype
    if out is None:
        out = torch.empty(shape, dtype=dt_out, device=dev)
    elif out.numel() != B * 3 * hp * wp or out.dtype != dt_out or not out.is_contiguous() or out.device != dev:
        raise L.OmgHipError(f"image_prep: out is a contiguous {dt_out} tensor of {shape} on the image's device, got {out.dtype} {tuple(out.shape)}")
    else:
        out = out.view(shape)
    lib = L.lib()
    src = u8
    if ow != W:
        bx, cx = ip.device_tables(W, ow, resample, dev)
        direct = oh == H and lut is None                       # the horizontal pass is the whole resize: straight into the result
        mid = out if direct else torch.empty((B, H, ow, 3), dtype=torch.uint8, device=dev)
        L.check(lib.omg_image_resize_h(B, H, W, ow, src.data_ptr(), bx.data_ptr(), cx.data_ptr(), cx.shape[1], mid.data_ptr(), _stream()),
                "omg_image_resize_h")
        if direct:
            return out if batched else out[0]
        src = mid
    if oh != H:
        by, cy = ip.device_tables(H, oh, resample, dev)
        pb, pc, ks = by.data_ptr(), cy.data_ptr(), cy.shape[1]
    else:
        pb, pc, ks = None, None, 0
    L.check(lib.omg_image_resize_v(B, H, ow, oh, src.data_ptr(), pb, pc, ks, code, _p(lut), hp, wp, out.data_ptr(), _stream()),
            "omg_image_resize_v")
    return out if batched else out[0]


# ------------------------------------------------------------------ Canny edge condition (omg_amd/canny.py has the arithmetic)
def _canny_u8(what: str, t, dims: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise L.OmgHipError(f"{what} takes a contiguous cuda uint8 {dims} tensor, got {type(t).__name__}")
    if not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() == 0:
        raise L.OmgHipError(f"{what} takes a contiguous cuda uint8 {dims} tensor, got {t.dtype} {tuple(t.shape)} on {t.device}"
                            f"{'' if t.is_contiguous() else ', not contiguous'}")


def _canny_thresholds(what: str, t1, t2) -> Tuple[int, int]:
    from . import canny as cn
    try:
        return cn.thresholds(t1, t2)
    except (TypeError, ValueError) as e:
        raise L.OmgHipError(f"{what}: thresholds ({t1!r}, {t2!r}): {e}") from None


def canny_nms(u8: torch.Tensor, low, high) -> torch.Tensor:
    """Sobel gradients, channel selection and non-maximum suppression of ``cv2.Canny`` in one launch (omg_canny_nms): a contiguous cuda
    uint8 ``[H, W]``, ``[H, W, C]`` or ``[B, H, W, C]`` image (C 1 or 3) -> the uint8 state map ``[H, W]`` / ``[B, H, W]``: 0 not an edge,
    1 kept and weak (``mag <= high``), 2 kept and strong.  ``low`` / ``high``: cv2's two thresholds (swapped if need be, floored)."""
    dims = "[H, W], [H, W, C] or [B, H, W, C] (C 1 or 3)"
    _canny_u8("canny_nms", u8, dims)
    if u8.dim() not in (2, 3, 4) or (u8.dim() >= 3 and u8.shape[-1] not in (1, 3)):
        raise L.OmgHipError(f"canny_nms takes a contiguous cuda uint8 {dims} tensor, got {tuple(u8.shape)}"
                            + (f": C = {u8.shape[-1]}" if u8.dim() >= 3 else ""))
    lo, hi = _canny_thresholds("canny_nms", low, high)
    Cn = 1 if u8.dim() == 2 else int(u8.shape[-1])
    B = int(u8.shape[0]) if u8.dim() == 4 else 1
    H, W = (int(u8.shape[0]), int(u8.shape[1])) if u8.dim() == 2 else (int(u8.shape[-3]), int(u8.shape[-2]))
    state = torch.empty((B, H, W) if u8.dim() == 4 else (H, W), dtype=torch.uint8, device=u8.device)
    L.check(L.lib().omg_canny_nms(B, H, W, Cn, u8.data_ptr(), lo, hi, state.data_ptr(), _stream()), "omg_canny_nms")
    return state


def canny_hysteresis(state: torch.Tensor, channels: int = 1, out_dtype: Optional[torch.dtype] = None, check: bool = True) -> torch.Tensor:
    """Hysteresis of ``cv2.Canny`` on a state map (omg_canny_hysteresis): a contiguous cuda uint8 ``[H, W]`` / ``[B, H, W]`` map of 0, 1
    and 2 -> the pixels of non-zero state whose 8-connected component holds a 2.  ``out_dtype`` None or uint8: uint8 0 / 255,
    ``[(B,) H, W]`` (``channels=1``) or ``[(B,) H, W, 3]`` (``channels=3``: the same byte three times); float16 / bfloat16 / float32: planar
    ``[(B,) 3, H, W]`` of 0 and 1.  Four launches and a workspace allocated per call, no host synchronisation: capturable.  ``check``
    reads the map's maximum back to refuse a value above 2; it is skipped while a graph is being captured."""
    _canny_u8("canny_hysteresis", state, "[H, W] or [B, H, W] state map")
    if state.dim() not in (2, 3):
        raise L.OmgHipError(f"canny_hysteresis takes a contiguous cuda uint8 [H, W] or [B, H, W] state map, got {tuple(state.shape)}")
    if channels not in (1, 3):
        raise L.OmgHipError(f"canny_hysteresis: channels={channels!r}, expected 1 or 3")
    planar = out_dtype is not None and out_dtype != torch.uint8
    if planar and out_dtype not in _LUT_DT:
        raise L.OmgHipError(f"canny_hysteresis: out_dtype {out_dtype}, expected uint8 (or None), float16, bfloat16 or float32")
    if check and not torch.cuda.is_current_stream_capturing():
        top = int(state.max())
        if top > 2:
            raise L.OmgHipError(f"canny_hysteresis: the state map holds the value {top}; states are 0 (none), 1 (weak) and 2 (strong)")
    batched = state.dim() == 3
    B = int(state.shape[0]) if batched else 1
    H, W = int(state.shape[-2]), int(state.shape[-1])
    if planar:
        form, code, shape, dt = 2, _LUT_DT[out_dtype], (B, 3, H, W), out_dtype
    elif channels == 3:
        form, code, shape, dt = 1, 0, (B, H, W, 3), torch.uint8
    else:
        form, code, shape, dt = 0, 0, (B, H, W), torch.uint8
    lib = L.lib()
    nbytes = int(lib.omg_canny_hysteresis_ws_bytes(B, H, W))
    if nbytes <= 0:
        raise L.OmgHipError(f"canny_hysteresis: sizes {(B, H, W)}: B <= 65535, H <= 16 * 65535 and B H W < 2^29")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=state.device)          # per call: see _gn_workspace
    out = torch.empty(shape, dtype=dt, device=state.device)
    L.check(lib.omg_canny_hysteresis(B, H, W, state.data_ptr(), ws.data_ptr(), form, code, out.data_ptr(), _stream()), "omg_canny_hysteresis")
    return out if batched else out[0]


def canny(u8: torch.Tensor, threshold1, threshold2, channels: int = 1, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``cv2.Canny(image, threshold1, threshold2)`` (apertureSize 3, L1 gradient) of a contiguous cuda uint8 ``[H, W]``, ``[H, W, C]`` or
    ``[B, H, W, C]`` image: canny_nms then canny_hysteresis, five launches, nothing on the host.  The output forms are canny_hysteresis's."""
    return canny_hysteresis(canny_nms(u8, threshold1, threshold2), channels=channels, out_dtype=out_dtype, check=False)


# ------------------------------------------------------------------ LoRA bank build: weight-slot merge
_LORA_KINDS = {"plain": L.LORA_PLAIN, "hada": L.LORA_HADA, "kron": L.LORA_KRON}


def _lora_desc(term: dict, N: int, K: int) -> "L.LoraTermDesc":
    """One term ``{"kind", "f", "s", "gain"}`` -> the C descriptor, shapes checked here so that the kernel reads inside its operands:
    plain ``f = (up [N, r], down [r, K])``; hada ``f = (w1_a [N, r], w1_b [r, K], w2_a [N, r2], w2_b [r2, K])``; kron
    ``f = (w1 [a, b], w2 [c, taps, d])`` with ``a c == N`` and ``taps b d == K``.  Factors are fp32, contiguous, on the device."""
    kind, f = term["kind"], term["f"]
    if kind not in _LORA_KINDS:
        raise L.OmgHipError(f"unknown LoRA term kind {kind!r}")
    for t in f:
        _dev(t)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise L.OmgHipError("LoRA term factors must be contiguous fp32 tensors")
    d = L.LoraTermDesc()
    d.kind, d.s = _LORA_KINDS[kind], float(term.get("s", 1.0))
    if kind == "plain":
        up, down = f
        if up.dim() != 2 or down.dim() != 2 or up.shape[0] != N or down.shape[1] != K or up.shape[1] != down.shape[0] or up.shape[1] < 1:
            raise L.OmgHipError(f"plain LoRA term: up {tuple(up.shape)} / down {tuple(down.shape)} do not give [{N}, {K}] (a zero-width stack is refused)")
        d.r = up.shape[1]
    elif kind == "hada":
        a1, b1, a2, b2 = f
        for a, b in ((a1, b1), (a2, b2)):
            if a.dim() != 2 or b.dim() != 2 or a.shape[0] != N or b.shape[1] != K or a.shape[1] != b.shape[0] or a.shape[1] < 1:
                raise L.OmgHipError(f"hada LoRA term: {tuple(a.shape)} . {tuple(b.shape)} does not give [{N}, {K}]")
        d.r, d.r2 = a1.shape[1], a2.shape[1]
    else:
        w1, w2 = f
        if w1.dim() != 2 or w2.dim() != 3 or w1.shape[0] * w2.shape[0] != N or w2.shape[1] * w1.shape[1] * w2.shape[2] != K or min(w1.shape + w2.shape) < 1:
            raise L.OmgHipError(f"kron LoRA term: w1 {tuple(w1.shape)} (x) w2 [c, taps, d] {tuple(w2.shape)} does not give [{N}, {K}]")
        d.a, d.b, d.c, d.taps, d.d = w1.shape[0], w1.shape[1], w2.shape[0], w2.shape[1], w2.shape[2]
    for i, t in enumerate(f):
        setattr(d, f"f{i}", t.data_ptr())
    g = term.get("gain")
    if g is not None:
        _dev(g)
        if g.dtype != torch.float32 or not g.is_contiguous() or tuple(g.shape) != (N,):
            raise L.OmgHipError(f"LoRA term gain must be a contiguous fp32 [{N}]")
        d.gain = g.data_ptr()
    return d


def _lora_w(w: torch.Tensor):
    _dev(w)
    if w.dim() != 2 or not w.is_contiguous() or w.shape[1] % 8 or w.shape[1] < 8 or w.shape[0] < 1:
        raise L.OmgHipError(f"LoRA merge needs a contiguous 16-bit [N, K] weight with K a multiple of 8, got {tuple(w.shape)}")
    return _dt(w), w.shape[0], w.shape[1]


def lora_rownorm(w: torch.Tensor, term: dict) -> torch.Tensor:
    """fp32 ``norm[n] = ||w[n, :] + s * delta[n, :]||_2`` of one term (omg_lora_rownorm): DoRA's weight norm, deterministic."""
    dt, N, K = _lora_w(w)
    d = _lora_desc(dict(term, gain=None), N, K)
    out = torch.empty(N, dtype=torch.float32, device=w.device)
    L.check(L.lib().omg_lora_rownorm(dt, N, K, w.data_ptr(), d, out.data_ptr(), _stream()), "omg_lora_rownorm")
    return out


def lora_merge_args(w: torch.Tensor, terms: Sequence[dict], out: torch.Tensor) -> "L.LoraMergeArgs":
    """The checked argument block of one ``omg_lora_merge`` launch (the caller keeps ``w``, ``out`` and the terms' tensors alive)."""
    dt, N, K = _lora_w(w)
    _dev(out)
    if out.dtype != w.dtype or tuple(out.shape) != (N, K) or not out.is_contiguous():
        raise L.OmgHipError("lora_merge: out must be a contiguous [N, K] view of the weight's dtype")
    if len(terms) > L.LORA_MAX_TERMS:
        raise L.OmgHipError(f"lora_merge: {len(terms)} terms, at most {L.LORA_MAX_TERMS} per slot and layer")
    a = L.LoraMergeArgs()
    a.dtype, a.N, a.K, a.n_terms, a.W, a.out = dt, N, K, len(terms), w.data_ptr(), out.data_ptr()
    for i, t in enumerate(terms):
        a.terms[i] = _lora_desc(t, N, K)
    return a


def lora_merge(w: torch.Tensor, terms: Sequence[dict], out: torch.Tensor) -> None:
    """``out[N, K] = round16(w * (1 + sum_t (gain_t - 1)) + sum_t gain_t * s_t * delta_t)`` (omg_lora_merge): one slot of a weight stack
    from the 16-bit base and up to four term descriptors, all arithmetic in fp32, no dense delta in memory."""
    L.check(L.lib().omg_lora_merge(lora_merge_args(w, terms, out), _stream()), "omg_lora_merge")
