"""Constructed inputs of the MX-fp8 quantiser tests (tests/test_oracle_mx8.py, tests/test_mx8_quantisers_gpu.py).

A block of 32 is one ANCHOR (the block's amax, which fixes the scale) plus 31 PROBES (|probe| <= anchor).  Everything is built
as 16-bit patterns of the input type, so that ties, e4m3 subnormals and underflow are placed and not left to chance:

* anchors, per binade of the input type (subnormal binades included): mantissa 1.0, 1.75 (amax / 448 is exactly a power of two),
  the patterns one ulp below and above 1.75, the all-ones mantissa — for fp16 that includes 65504;
* probes of an anchor: every pattern of both signs with magnitude in [anchor * 2^-14, anchor]; the e4m3 subnormal grid of the
  anchor's scale in quarter steps (j * 2^-11 * scale, j = 0 .. 36: every subnormal, every tie between two of them, the tie
  between zero and the smallest, the step into the normal range) with the input patterns one ulp either side; +-0; and a few
  patterns far below, which must come out as 0x00 / 0x80.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

MBITS = {torch.float16: 10, torch.bfloat16: 7}
EBIAS = {torch.float16: 15, torch.bfloat16: 127}
EMAX_FIELD = {torch.float16: 30, torch.bfloat16: 254}


def to_float(bits: np.ndarray, dtype) -> torch.Tensor:
    """uint16 patterns -> fp32 tensor of the values (exact)."""
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(dtype).float()


def to_tensor(bits: np.ndarray, dtype) -> torch.Tensor:
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(dtype)


def value(bits: int, dtype) -> float:
    """Positive pattern -> its value as a Python float (exact)."""
    mb, bias = MBITS[dtype], EBIAS[dtype]
    f, m = bits >> mb, bits & ((1 << mb) - 1)
    return math.ldexp(m, 1 - bias - mb) if f == 0 else math.ldexp((1 << mb) + m, f - bias - mb)


def pattern_floor(v: float, dtype) -> int:
    """The largest positive pattern whose value is <= v (v >= 0)."""
    mb, bias = MBITS[dtype], EBIAS[dtype]
    if v <= 0:
        return 0
    top = (EMAX_FIELD[dtype] << mb) | ((1 << mb) - 1)
    m, e = math.frexp(v)                                  # v = m 2^e, m in [0.5, 1)
    f = e - 1 + bias
    if f <= 0:
        return min(top, int(math.floor(math.ldexp(v, bias - 1 + mb))))
    return min(top, (f << mb) | int(math.floor(math.ldexp(m, mb + 1))) - (1 << mb))


def scale_exponent(anchor: int, dtype) -> int:
    """The contract, in exact arithmetic: the smallest e >= -127 with value(anchor) <= 448 * 2^e."""
    v = value(anchor, dtype)
    e = math.frexp(v)[1] - 9                              # a first guess; the two comparisons below are exact in float64
    while v <= math.ldexp(448.0, e - 1):
        e -= 1
    while v > math.ldexp(448.0, e):
        e += 1
    return max(e, -127)


@functools.lru_cache(maxsize=None)
def anchors(dtype) -> tuple:
    """Sorted positive anchor patterns of the input type."""
    mb = MBITS[dtype]
    out = set()
    for f in range(1, EMAX_FIELD[dtype] + 1):             # normal binades
        base = f << mb
        m175 = 3 << (mb - 2)
        out.update(base | m for m in (0, m175 - 1, m175, m175 + 1, (1 << mb) - 1))
    for k in range(mb):                                   # subnormal binades: leading bit k
        lead = 1 << k
        out.update((lead, 2 * lead - 1))
        if k >= 2:
            m175 = 7 << (k - 2)
            out.update((m175 - 1, m175, m175 + 1))
    return tuple(sorted(out))


def special_probes(anchor: int, dtype) -> np.ndarray:
    """Signed probe patterns around the e4m3 subnormal grid of the anchor's scale, +-0 and far-below values."""
    e = scale_exponent(anchor, dtype)
    pos = {0}
    for j in range(37):
        p = pattern_floor(math.ldexp(j, e - 11), dtype)  # exact where the input type can hold it
        pos.update((max(p - 1, 0), p, p + 1))
    for far in (24, 30, 40):
        pos.add(pattern_floor(math.ldexp(value(anchor, dtype), -far), dtype))
    pos = np.array(sorted(p for p in pos if p <= anchor), dtype=np.uint16)
    return np.concatenate([pos, pos | 0x8000])


def range_probes(anchor: int, dtype) -> np.ndarray:
    """Every pattern of both signs with magnitude in [anchor * 2^-14, anchor]."""
    lo = max(1, pattern_floor(math.ldexp(value(anchor, dtype), -14), dtype))
    pos = np.arange(lo, anchor + 1, dtype=np.uint16)
    return np.concatenate([pos, pos | 0x8000])


def blocks_of(anchor: int, probes: np.ndarray, first_block: int = 0) -> np.ndarray:
    """uint16 [n, 32]: the probes in blocks of 31 with the anchor rotated through the 32 positions (block i: position
    (first_block + i) % 32, sign negative on every other turn of the rotation); the last block is filled up with zeros."""
    n = (len(probes) + 30) // 31
    body = np.zeros(n * 31, dtype=np.uint16)
    body[:len(probes)] = probes
    body = body.reshape(n, 31)
    out = np.empty((n, 32), dtype=np.uint16)
    idx = np.arange(n) + first_block
    pos = idx % 32
    cols = np.arange(32)[None, :]
    src = cols - (cols > pos[:, None])                    # column c takes probe c (left of the anchor) or c - 1 (right of it)
    out[:] = np.take_along_axis(body, np.clip(src, 0, 30), axis=1)
    out[np.arange(n), pos] = np.uint16(anchor) | np.where((idx // 32) % 2 == 1, 0x8000, 0).astype(np.uint16)
    return out


def rows_of(blocks: np.ndarray, K: int = 128) -> np.ndarray:
    """uint16 [n, 32] -> [rows, K], filled up with blocks of zeros."""
    per = K // 32
    n = (len(blocks) + per - 1) // per * per
    full = np.zeros((n, 32), dtype=np.uint16)
    full[:len(blocks)] = blocks
    return full.reshape(n // per, K)


@functools.lru_cache(maxsize=None)
def every_element_sweep(dtype) -> torch.Tensor:
    """The whole sweep of one input type as [rows, 128] of that type."""
    parts = [blocks_of(a, np.concatenate([special_probes(a, dtype), range_probes(a, dtype)]), first_block=a) for a in anchors(dtype)]
    return to_tensor(rows_of(np.concatenate(parts)), dtype)


TINY_BF16_LAST = (9 << 7) | 0x60                         # 448 * 2^-126 = 1.75 * 2^-118: the top of the range whose scale byte is 1


@functools.lru_cache(maxsize=None)
def tiny_bf16_sweep() -> torch.Tensor:
    """One block per bf16 amax from 9.2e-41 (pattern 1) to 448 * 2^-126: patterns 1 .. 1120 have the clamped scale byte 0
    (amax <= 448 * 2^-127), patterns 1121 .. 1248 byte 1.  Probes: 31 patterns spread over [0, anchor], alternating sign."""
    blocks = []
    for a in range(1, TINY_BF16_LAST + 1):
        pr = (np.arange(31, dtype=np.int64) * a // 30).astype(np.uint16)
        pr[1::2] |= 0x8000
        blocks.append(blocks_of(a, pr, first_block=a))
    return to_tensor(rows_of(np.concatenate(blocks)), torch.bfloat16)


def chosen_blocks(dtype, nblocks: int, seed: int) -> np.ndarray:
    """uint16 [nblocks * 32] for the fused producers' beta: block j has a sampled anchor (the tiny-amax ones of bf16 and the
    format's extremes come first) at position (9 j) % 32 — lane j % 4 of the block's four lanes — and 31 probes, half of them
    from the subnormal / tie grid of the anchor's scale, half from the dense range below the anchor."""
    rng = np.random.RandomState(seed)
    al = anchors(dtype)
    forced = [al[-1], al[0]] + ([1120, 1121, TINY_BF16_LAST, TINY_BF16_LAST + 1, 700] if dtype == torch.bfloat16 else [0x03ff, 0x0400])
    order = rng.permutation(len(forced))
    out = np.zeros((nblocks, 32), dtype=np.uint16)
    for j in range(nblocks):
        a = forced[order[j]] if j < len(forced) else al[rng.randint(len(al))]
        sp, rp = special_probes(a, dtype), range_probes(a, dtype)
        pr = np.concatenate([sp[rng.randint(len(sp), size=15)], rp[rng.randint(len(rp), size=16)]])
        pos = (9 * j) % 32
        out[j, :pos] = pr[:pos]
        out[j, pos + 1:] = pr[pos:]
        out[j, pos] = a | (0x8000 if j % 3 == 2 else 0)
    return out.reshape(-1)


def describe_first_mismatch(x: torch.Tensor, got_q: torch.Tensor, want_q: torch.Tensor, got_b: torch.Tensor, want_b: torch.Tensor,
                            skip: torch.Tensor = None) -> str:
    """Readable report of the first differing element byte and the first differing scale byte.
    x [rows, K] 16-bit, *_q uint8 [rows, K], *_b scale BYTES [rows, K/32], skip bool [rows, K/32] (blocks left out)."""
    rows, K = x.shape
    bits = x.view(torch.int16).to(torch.int32) & 0xFFFF
    lines = []
    bad_q, bad_b = got_q != want_q, got_b != want_b
    if skip is not None:
        bad_q = bad_q & ~skip.repeat_interleave(32, dim=1)
        bad_b = bad_b & ~skip
    for name, bad in (("scale byte", bad_b), ("element byte", bad_q)):
        n = int(bad.sum())
        if n == 0:
            continue
        r, c = (int(v) for v in bad.nonzero()[0])
        blk = c if name == "scale byte" else c // 32
        blk_bits = bits[r, blk * 32:(blk + 1) * 32]
        amax_i = int(x[r, blk * 32:(blk + 1) * 32].float().abs().argmax())
        head = f"{n} {name}s differ; first at row {r}, block {blk}: amax pattern 0x{int(blk_bits[amax_i]):04x} ({float(x[r, blk * 32 + amax_i]):.6g}) at position {amax_i}"
        if name == "scale byte":
            lines.append(f"{head}: expected scale byte {int(want_b[r, c])}, received {int(got_b[r, c])}")
        else:
            lines.append(f"{head}, scale byte expected {int(want_b[r, blk])} received {int(got_b[r, blk])}; element {c % 32}: input pattern "
                         f"0x{int(bits[r, c]):04x} ({float(x[r, c]):.6g}): expected byte 0x{int(want_q[r, c]):02x}, received 0x{int(got_q[r, c]):02x}")
    return "\n".join(lines)


def scale_bytes(packed: torch.Tensor, rows: int) -> torch.Tensor:
    """int32 scale dwords [K/128, s_ld] -> uint8-valued int64 [rows, K/32]."""
    p = packed[:, :rows].t().to(torch.int64) & 0xFFFFFFFF
    return torch.stack([(p >> (8 * i)) & 0xFF for i in range(4)], dim=-1).reshape(rows, -1)
