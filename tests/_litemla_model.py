"""CPU references for LiteMLA's linear attention and depthwise convolution (csrc/litemla.hip): plain torch, no GPU.

Linear attention, per (sample, group of 3 dim channels):  kv = relu(K)^T [V | 1]  over all tokens, then per token
out = relu(q) kv,  out[:dim] / (out[dim] + eps).

  truth            the formula in float64 on the STORED 16-bit operands: the reference of record.
  ref32            the same formula evaluated by torch in fp32, unrounded, returned as float64: how far an fp32 evaluation is from
                   `truth` on this input (its conditioning), in the summation order torch happens to use.
  held             the rule of tests/test_litemla_conditioning_gpu.py.  Elementwise, no element excluded:

                       |out[i] - truth[i]|  <=  ulp16(truth[i]) / 2  +  C * E32

                   E32 = max |ref32 - truth| over the case, floored at 2^-23 max |truth| (the two fp32 roundings of o * (1 / den));
                   C = 4 is C_MAX of tests/test_attention_conditioning_gpu.py and allows for another fp32 summation order.  The first
                   term is the one rounding to the storage type.  `out` must be finite.
  rla_emulation    the kernel's own algorithm in fp32 (per-128-token partials summed token by token, partials added in chunk order,
                   q . kv channel by channel, one reciprocal), with one fault at a time: what tests/test_litemla_model.py uses to show
                   that `held` rejects a subtly wrong kernel.
  dwconv_emulation dwconv_kernel's order in fp32 from the stored operands: starts from bias (or 0) and adds x * w per tap, dy outer,
                   dx inner, out-of-image taps skipped.  The product of two fp16 values has 22 significant bits, of two bf16 values
                   16: exact in fp32 while it stays in the normal range (bf16 operands within 2^-20 .. 2^20), so fma(x, w, acc) is
                   acc + x * w rounded once and the kernel can be reproduced bit for bit.
"""
import torch
import torch.nn.functional as F

F16, BF16 = torch.float16, torch.bfloat16
C_RULE = 4.0
TCH = 128                       # RLA_TCH of litemla.hip: tokens per partial-sum chunk
FAMILIES = ("plain", "sparse_offset", "cancel", "wide")


def name(dtype):
    return "fp16" if dtype == F16 else "bf16"


def eps32(eps):
    """The value the kernel sees: eps is passed as a float."""
    return float(torch.tensor(eps, dtype=torch.float32))


def split(qkv, B, HW, G, dim):
    t = qkv.reshape(B, HW, G, 3 * dim).permute(0, 2, 1, 3)                       # (B, G, HW, 3 dim)
    return torch.relu(t[..., :dim]), torch.relu(t[..., dim:2 * dim]), t[..., 2 * dim:]


def _rows(o, B, HW, G, dim):
    return o.permute(0, 2, 1, 3).reshape(B * HW, G * dim)


def _formula(qkv, B, HW, G, dim, eps, ft):
    q, k, v = split(qkv.to(ft), B, HW, G, dim)
    v = F.pad(v, (0, 1), value=1.0)
    o = q @ (k.transpose(-1, -2) @ v)
    return _rows(o[..., :-1] / (o[..., -1:] + torch.tensor(eps32(eps), dtype=ft)), B, HW, G, dim)


def truth(qkv, B, HW, G, dim, eps):
    return _formula(qkv, B, HW, G, dim, eps, torch.float64)


def ref32(qkv, B, HW, G, dim, eps):
    return _formula(qkv, B, HW, G, dim, eps, torch.float32).double()


def ulp16(t, dtype):
    """Elementwise spacing of `dtype` at |t|: 2^(floor(log2 |t|) - 10) for fp16, - 7 for bf16; the exponent floored at the smallest
    normal one (-14, -126), which is also the spacing of the subnormals."""
    bits, emin = (10, -14) if dtype == F16 else (7, -126)
    e = torch.floor(torch.log2(t.double().abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - bits)


def held(tag, dtype, out, truth, ref32, log=None, allow=None):
    """Applies the rule to one case (`allow`, if given, is a further elementwise term of the bound: tests/_conv3x3_model.py); what it measured goes to `log` (a list) before it asserts.  Figures: E32; the excess of the error
    over the half ulp, over E32 (a lower bound of the kernel's fp32 error over E32, which a 16-bit output does not show directly); the
    error over the rule's bound; the share of elements that are not round16(truth)."""
    out = out.detach().cpu()
    finite = bool(torch.isfinite(out).all())
    o = out.double()
    tmax = float(truth.abs().max()) if truth.numel() else 0.0
    E32 = max(float((ref32 - truth).abs().max()) if truth.numel() else 0.0, 2.0 ** -23 * tmax)
    err = (o - truth).abs()
    half = ulp16(truth, dtype) / 2
    bound = half + C_RULE * E32 if allow is None else half + C_RULE * E32 + allow
    excess = (err - half).clamp_min(0)
    rec = dict(tag=tag, dtype=name(dtype), E32=E32, max_truth=tmax, finite=finite,
               excess_over_E32=(float(torch.nan_to_num(excess, nan=float("inf")).max()) / E32 if E32 > 0 else 0.0) if truth.numel() else 0.0,
               err_over_bound=float(torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf")).max()) if truth.numel() else 0.0,
               not_round_truth=float((o != truth.to(dtype).double()).double().mean()) if truth.numel() else 0.0)
    if log is not None:
        log.append(rec)
    assert finite, f"{tag}: non-finite output"
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))))
        r, c = divmod(i, truth.shape[1])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements break the rule; worst at row {r} column {c}: out {float(o[r, c])!r} "
                             f"truth {float(truth[r, c])!r} error {float(err[r, c]):.3e} > ulp/2 {float(half[r, c]):.3e} + {C_RULE} * E32 {E32:.3e}"
                             + ("" if allow is None else f" + allowance {float(allow[r, c]):.3e}"))
    return rec


def family(kind, B, HW, G, dim, seed):
    """The input families of the conditioning tests as fp32 [B*HW, G*3*dim] (the caller rounds to the storage type).
    plain: randn.  sparse_offset: q and k shifted by -1.5 (few ReLU survivors, dead query rows), v = 100 + randn / 4 (a large common
    offset).  cancel: v = +-64 alternating by token plus randn / 10, so kv cancels.  wide: each token's k scaled by 2^u, u in -8..8."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * HW, G, 3 * dim, generator=g)
    if kind == "sparse_offset":
        x[..., :2 * dim] -= 1.5
        x[..., 2 * dim:] = x[..., 2 * dim:] * 0.25 + 100.0
    elif kind == "cancel":
        sgn = (torch.arange(B * HW) % HW % 2 * 2 - 1).float()[:, None, None]
        x[..., 2 * dim:] = sgn * 64.0 + x[..., 2 * dim:] * 0.1
    elif kind == "wide":
        x[..., dim:2 * dim] *= torch.exp2(torch.randint(-8, 9, (B * HW, 1, 1), generator=g).float())
    else:
        assert kind == "plain", kind
    return x.reshape(B * HW, G * 3 * dim)


def dead_and_live_rows(qkv, B, HW, G, dim):
    """Shares of (token, group) rows whose relu(q) is 0 in every channel, and of rows whose float64 result is not all zero."""
    q, _, _ = split(qkv.double(), B, HW, G, dim)
    t = truth(qkv, B, HW, G, dim, 1e-15).reshape(B * HW, G, dim)
    return float((q.amax(-1) == 0).double().mean()), float((t.abs().amax(-1) > 0).double().mean())


RLA_FAULTS = ("no_eps", "kv_transposed", "relu_v", "ones_padded", "skip_last_chunk", "k_next_group")


def rla_emulation(qkv, B, HW, G, dim, eps, fault=None):
    """rla_kv_kernel + rla_apply_kernel in fp32, unrounded, as float64 [B*HW, G*dim].  k * v is exact in fp32, so the chunk sums are the
    kernel's fma chain; q * kv is not, so that fma is taken in float64 and rounded to fp32 (a double rounding, rare and 2^-53 relative).
    Faults: no_eps (eps never added); kv_transposed (kv[j][i] for kv[i][j]); relu_v; ones_padded (the padded tokens of the last chunk
    repeat the last token's k with v = 0 and are counted in the "1" column: with k = 0, as the kernel has it, the 1 alone is harmless);
    skip_last_chunk; k_next_group (k read from group g + 1, cyclically)."""
    assert fault is None or fault in RLA_FAULTS, fault
    q, k, v = split(qkv.float(), B, HW, G, dim)
    if fault == "relu_v":
        v = torch.relu(v)
    if fault == "k_next_group":
        k = torch.roll(k, -1, dims=1)
    v = F.pad(v, (0, 1), value=1.0)
    nch = (HW + TCH - 1) // TCH
    kv = torch.zeros(B, G, dim, dim + 1)
    for c in range(nch):
        if fault == "skip_last_chunk" and c == nch - 1:
            continue
        part = torch.zeros(B, G, dim, dim + 1)
        for t in range(c * TCH, min(HW, (c + 1) * TCH)):
            part = part + k[:, :, t, :, None] * v[:, :, t, None, :]
        if fault == "ones_padded":
            for t in range(HW, (c + 1) * TCH):
                part[..., dim] = part[..., dim] + k[:, :, HW - 1, :]
        kv = kv + part
    if fault == "kv_transposed":
        kv = torch.cat([kv[..., :dim].transpose(-1, -2), kv[..., dim:]], -1)
    o = torch.zeros(B, G, HW, dim + 1)
    for i in range(dim):
        o = (o.double() + q[..., i, None].double() * kv[:, :, None, i, :].double()).float()
    den = o[..., -1:] if fault == "no_eps" else o[..., -1:] + torch.tensor(eps32(eps), dtype=torch.float32)
    inv = 1.0 / den
    return _rows(o[..., :-1] * inv, B, HW, G, dim).double()


DW_FAULTS = ("swap_dy_dx", "wrap_batch", "bias_after_round")


def dwconv_emulation(x, taps, bias, B, H, W, k, fault=None):
    """dwconv_kernel in fp32, unrounded: x [B*H*W, C] NHWC rows and taps [k*k, C] of a 16-bit type, bias [C] or None -> fp32 [B*H*W, C];
    `.to(x.dtype)` is what the kernel stores.  Faults (for tests/test_litemla_model.py; these return the ROUNDED result as fp32):
    swap_dy_dx (tap (dy, dx) takes the weight of (dx, dy)); wrap_batch (a tap that leaves the image vertically reads the neighbouring
    image of the batch); bias_after_round (bias added to the rounded sum, rounded again)."""
    assert fault is None or fault in DW_FAULTS, fault
    C = x.shape[1]
    xf, tf, r = x.float().reshape(B, H, W, C), taps.float(), k // 2
    late = fault == "bias_after_round"
    acc = (bias.float() if bias is not None and not late else torch.zeros(C)).expand(B, H, W, C).clone()
    if fault == "wrap_batch":
        xf, acc = xf.reshape(1, B * H, W, C), acc.reshape(1, B * H, W, C)
    Hh = xf.shape[1]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y0, y1, x0, x1 = max(0, -dy), min(Hh, Hh - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            w = tf[(dx + r) * k + dy + r] if fault == "swap_dy_dx" else tf[(dy + r) * k + dx + r]
            acc[:, y0:y1, x0:x1] = acc[:, y0:y1, x0:x1] + xf[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx] * w
    acc = acc.reshape(B * H * W, C)
    if fault is None:
        return acc
    if late and bias is not None:
        acc = acc.to(x.dtype).float() + bias.float()
    return acc.to(x.dtype).float()


def dwconv_inputs(B, H, W, C, k, dtype, seed, with_bias=True):
    """x [B*H*W, C], taps [k*k, C] (randn / k), bias [C] in `dtype`; magnitudes below 2^-10 are raised to 2^-10 so that every product is
    exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    def away_from_zero(t):
        return torch.where(t.abs() < 2.0 ** -10, torch.full_like(t, 2.0 ** -10), t).to(dtype)
    x = away_from_zero(torch.randn(B * H * W, C, generator=g))
    taps = away_from_zero(torch.randn(k * k, C, generator=g) / k)
    bias = away_from_zero(torch.randn(C, generator=g)) if with_bias else None
    return x, taps, bias
