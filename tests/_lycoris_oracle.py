"""Float64 model of the LoHa / LoKr / DoRA weight merge, shared by tests/test_lycoris.py (CPU), tests/test_lora_merge_gpu.py and
tests/test_lycoris_gpu.py.  Written independently of omg_amd/loaders.py and omg_amd/lora.py: the deltas are ``torch.kron`` and explicit
reshapes of the file tensors, nothing here calls the product.

Deltas (file layout, ``shape`` = the base weight's ``[out, in]`` or ``[out, in, k, k]``):

    plain   up [out, r] . down [r, in k k]                                  reshaped to ``shape``
    hada    (w1_a . w1_b) * (w2_a . w2_b)                                   reshaped to ``shape``
    kron    torch.kron(w1 [a, b, (1, 1)], w2 [c, d, (k, k)])               delta[ia c + ic, ib d + id, ky, kx] = w1[ia, ib] w2[ic, id, ky, kx]

The slot (PEFT's rule for several active adapters, each with its own norm; ``g_a = 1`` without a magnitude):

    n_a = || W + s_a delta_a ||_2 over every axis but the output's (no epsilon),   g_a = m_a / n_a
    W_slot = round16( W (1 + sum_a (g_a - 1)) + sum_a g_a s_a delta_a )

The error bound of the merge kernel, per element, with u32 = 2^-24 and S the sum of the absolute values of all products entering it
(``|W| (1 + sum_a |g_a - 1|) + sum_a |g_a s_a| sum_q |factor products|``):

    |got - exact| <= 1/2 ulp16(max(|got|, |exact|)) + C (r + 2) u32 S,      C = 4,  r = the largest rank of the element's terms

C = 4, first order in u32: a rank-r fmaf chain is off by at most r u32 of its absolute sum; a LoHa element is the rounded product of two
chains, (2 r + 1) u32; g s is one rounding more: (2 r + 2) u32 on a term's part of S.  On W's part: g_a - 1 one rounding each, their sum with
1 at most T = 4 more, the product with W one: (T + 2) u32.  Adding the T terms to the accumulator rounds T partial sums, each at most S: T u32
on all of S.  Together at most (max(2 r + 2, T + 2) + T) u32 S = max(2 r + 6, 10) u32 S <= 4 (r + 2) u32 S for every r >= 1; the second-order
terms are below 1e-6 of that.  Nothing is excluded from the comparison.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import torch

U32 = 2.0 ** -24
C = 4.0
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}


# ------------------------------------------------------------------ deltas, float64
def kron_operand(full: Optional[torch.Tensor], a: Optional[torch.Tensor] = None, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A LoKr operand: the full matrix, or ``a . b`` (a 4-D w2 comes back as ``[c, d k k]``; :func:`delta` reshapes it)."""
    return full.double() if full is not None else a.double() @ b.double()


def delta(kind: str, f: Sequence[torch.Tensor], shape: Sequence[int], absolute: bool = False) -> torch.Tensor:
    """The dense float64 delta in the base weight's shape; ``absolute=True``: the same with every factor replaced by its absolute value
    (the sum of the absolute products, S's ingredient)."""
    f = [t.double().abs() if absolute else t.double() for t in f]
    out = shape[0]
    if kind == "plain":
        down, up = f
        return (up.reshape(out, -1) @ down.reshape(down.shape[0], -1)).reshape(*shape)
    if kind == "hada":
        w1a, w1b, w2a, w2b = f
        return ((w1a @ w1b) * (w2a @ w2b)).reshape(*shape)
    if kind == "kron":
        w1, w2 = f
        if len(shape) == 4:
            c, d = out // w1.shape[0], shape[1] // w1.shape[1]
            return torch.kron(w1[:, :, None, None].contiguous(), w2.reshape(c, d, shape[2], shape[3]))
        return torch.kron(w1, w2)
    raise ValueError(kind)


def pack(w: torch.Tensor) -> torch.Tensor:
    """[out, in, k, k] -> [out, (ky, kx, in)], the column order of the engine's convolution weights; a Linear's [out, in] unchanged."""
    return w if w.dim() == 2 else w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


# ------------------------------------------------------------------ the slot, float64, with the deliberate defects of the self-check
FAULTS = ("s_outside_norm", "norm_over_output", "kron_swapped", "conv_cin_order", "alpha_dropped", "gm1_dropped", "joint_norm")


def slot_weight(W: torch.Tensor, terms: Sequence[dict], fault: Optional[str] = None, packed: bool = True) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """``terms`` = [{"kind", "f" (file layout, fp32), "scale" (slot scale x adapter weight), "factor" (alpha / r), "m" ([out] or None),
    "r"}].  Returns ``(exact, S, r)`` before the 16-bit rounding: in the engine's packed ``[out, K]`` column order, or with
    ``packed=False`` in the base weight's own shape (a state-dict entry)."""
    W = W.double()
    red = tuple(range(1, W.dim()))
    bc = lambda v: v.reshape(-1, *([1] * (W.dim() - 1)))
    ds, ss, ab = [], [], []
    for t in terms:
        f = list(t["f"])
        if fault == "kron_swapped" and t["kind"] == "kron":
            w1, w2 = f[0].double(), f[1].double()
            if W.dim() == 4:
                w1, w2 = w1[:, :, None, None].contiguous(), w2.reshape(W.shape[0] // w1.shape[0], W.shape[1] // w1.shape[1], W.shape[2], W.shape[3])
            d = torch.kron(w2, w1)
        else:
            d = delta(t["kind"], f, W.shape)
        ds.append(d)
        ab.append(delta(t["kind"], t["f"], W.shape, absolute=True))
        ss.append(float(t["scale"]) * (1.0 if fault == "alpha_dropped" else float(t["factor"])))
    joint = W + sum(s * d for s, d in zip(ss, ds)) if terms else W
    wcoef, acc, S = torch.ones(W.shape[0], dtype=torch.float64), torch.zeros_like(W), torch.zeros_like(W)
    wabs = torch.ones(W.shape[0], dtype=torch.float64)
    for t, d, s, a in zip(terms, ds, ss, ab):
        g = torch.ones(W.shape[0], dtype=torch.float64)
        if t.get("m") is not None:
            v = joint if fault == "joint_norm" else (W + d if fault == "s_outside_norm" else W + s * d)
            if fault == "norm_over_output":
                cols = v.reshape(W.shape[0], -1).pow(2).sum(0).sqrt()          # one norm per input column, handed out to the rows in turn
                n = cols[torch.arange(W.shape[0]) % cols.numel()]
            else:
                n = v.pow(2).sum(red).sqrt()
            g = t["m"].double().reshape(-1) / n
        if fault != "gm1_dropped":
            wcoef = wcoef + (g - 1)
        wabs = wabs + (g - 1).abs()
        acc = acc + bc(g) * s * d
        S = S + bc(g.abs()) * abs(s) * a
    exact = W * bc(wcoef) + acc
    S = S + W.abs() * bc(wabs)
    if fault == "conv_cin_order" and W.dim() == 4:               # columns left in (Cin, ky, kx) order where the engine wants (ky, kx, Cin)
        return exact.reshape(W.shape[0], -1), pack(S), max(t["r"] for t in terms)
    r = max([t["r"] for t in terms] or [1])
    return (pack(exact), pack(S), r) if packed else (exact, S, r)


def gain_slack(W: torch.Tensor, terms: Sequence[dict]) -> torch.Tensor:
    """Per output channel, the sum over the terms with a magnitude of the relative error a gain m / n may carry when n comes from the norm
    kernel: the norm's own bound (:func:`rownorm_exact`) over the norm, plus one rounding for the division and one for m in fp32.  A
    slot built with such gains is within ``bound + gain_slack[:, None] * S`` of :func:`slot_weight`."""
    Wp = pack(W.double())
    eps = torch.zeros(W.shape[0], dtype=torch.float64)
    for t in terms:
        if t.get("m") is None:
            continue
        d, a = pack(delta(t["kind"], t["f"], W.shape)), pack(delta(t["kind"], t["f"], W.shape, absolute=True))
        n, nb = rownorm_exact(Wp, d, a, float(t["scale"]) * float(t["factor"]), t["r"])
        eps = eps + nb / n + 2 * U32
    return eps


# ------------------------------------------------------------------ the kernel's own formula: gains given, packed [N, K]
def merge_exact(W: torch.Tensor, terms: Sequence[dict]) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """``terms`` = [{"d": delta [N, K] float64, "a": absolute-product sum [N, K], "s": float, "gain": fp32 [N] or None, "r"}]; ``s`` is taken
    through fp32 as the C ABI does.  Returns ``(exact, S, r)``."""
    W = W.double()
    wcoef, wabs = torch.ones(W.shape[0], dtype=torch.float64), torch.ones(W.shape[0], dtype=torch.float64)
    acc, S = torch.zeros_like(W), torch.zeros_like(W)
    for t in terms:
        s = float(torch.tensor(t["s"], dtype=torch.float32))
        g = torch.ones(W.shape[0], dtype=torch.float64) if t.get("gain") is None else t["gain"].double().cpu()
        wcoef, wabs = wcoef + (g - 1), wabs + (g - 1).abs()
        acc = acc + g[:, None] * s * t["d"]
        S = S + g.abs()[:, None] * abs(s) * t["a"]
    return W * wcoef[:, None] + acc, S + W.abs() * wabs[:, None], max([t["r"] for t in terms] or [1])


def rownorm_exact(W: torch.Tensor, d: torch.Tensor, a: torch.Tensor, s: float, r: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(norm, bound)`` of ``||W + s d||`` per row.  Bound, first order: an element v = fma(s, d, W) is off by at most (2 r + 2) u32 V,
    V = |W| + |s| a (the chain(s), their product, the fma); the sum of K squares in any order by at most K u32 of itself; the root by one
    rounding: |n - exact| <= u32 ((2 r + 2) sum V^2 / n + (K / 2 + 2) n), doubled for the second-order terms."""
    s = float(torch.tensor(s, dtype=torch.float32))
    v = W.double() + s * d
    n = v.pow(2).sum(1).sqrt()
    V = W.double().abs() + abs(s) * a
    K = W.shape[1]
    bound = 2 * U32 * ((2 * r + 2) * V.pow(2).sum(1) / n.clamp_min(1e-300) + (K / 2 + 2) * n)
    return n, bound


# ------------------------------------------------------------------ the bound
def ulp16(x: torch.Tensor, dtype) -> torch.Tensor:
    """The spacing of ``dtype`` at |x| (float64 in, float64 out); the subnormal spacing below the smallest normal number."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** EMIN[dtype]))).clamp_min(EMIN[dtype])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dtype])


def bound(got: torch.Tensor, exact: torch.Tensor, S: torch.Tensor, r: int, dtype) -> torch.Tensor:
    return 0.5 * ulp16(torch.maximum(got.abs(), exact.abs()), dtype) + C * (r + 2) * U32 * S


def held(got16: torch.Tensor, exact: torch.Tensor, S: torch.Tensor, r: int) -> Tuple[bool, float]:
    """``(every element within the bound, the largest |error| / bound)`` of a 16-bit result against the float64 one."""
    got = got16.double().cpu()
    ratio = (got - exact).abs() / bound(got, exact, S, r, got16.dtype)
    return bool((ratio <= 1.0).all()) and bool(torch.isfinite(got).all()), float(ratio.max())
