"""Attention kernels (csrc/attn.hip: v2, v6; csrc/attn_v7.h: v7; the protocol-mode pair) at every key / query edge, bounded
by a rounding model instead of a fixed tolerance (-m gpu).

References (tests/_attn_model.py, CPU float64, on the STORED 16-bit inputs): `truth` = softmax(q k^T scale) v, the reference
of record; `model` = the same with the design's rounding points only (Q' = round16(fp32(q) * scale log2 e), exact scores,
P = round16(exp2(S - rowmax)), O = P v / sum P, rounded once to the storage type).  With e_k = |kernel - truth| and
e_m = |model - truth| over the WHOLE output of a case, a case passes when

    max(e_k) <= max(FLOOR, C_MAX * max(e_m))   and   rms(e_k) <= max(FLOOR_RMS, C_RMS * rms(e_m))

FLOOR = one ulp of the storage type at the case's largest |truth| (the output rounding), FLOOR_RMS = FLOOR / sqrt(12).
The kernels realise the model's roundings at other values (P relative to a lazy reference up to 2^8 above the row maximum,
the hardware's exp2, fp32 sums in MFMA order), so their error is another draw from the model's distribution: C_MAX and C_RMS
are twice the worst ratio measured on the MI355X over all cases of sections 1 - 3, rounded up to one digit, and never above 4
(see MEASURED below; profiles/r08_attention_conditioning.log is the module's own output: per key count the worst case over
its query counts, kernels and forms, with that case's figures).

1. Every edge: key counts around every 16-key block of the cross-attention tile (1 .. 128; v6, and v2 forced, which must be
   bitwise v6) with query counts around the 32-row wave, the 128-row step and the 512-row strip; key counts around the
   64-key tile above 128 (v7 on row-major V, v2 on a V^T image) with query counts around v7's 64-row wave and 256-row
   workgroup, grids of 4 (not a multiple of 8) and 8 blocks (the XCD-aware order); plain, borrowed Q / K (qk_src),
   accumulate with out_scale 0.8; input scale 1.2 and 3.0.
2. Exact answers: V[key, d] = (d == key % 64), so column d is the probability mass of the keys congruent to d.  q = 0: every
   output is count(d) / Nkv to one ulp.  One dominant key per query row (q_j = 4 k[j % Nkv]): row j is the one-hot of
   (j % Nkv) % 64, every position of every 16-key group of every tile once, the ragged tail included; the same with
   V[key, d] = key // 64, which tells tiles apart.
3. The lazy reference maximum (ATTN_THR = 8) under prescribed logits: scale = ln 2 makes Q' = q, and q = a u + b w,
   k = c u + n w with u, w orthogonal unit vectors of entries +-1/4 makes the log2-unit logit exactly a c + b n.  A raise
   in every tile, none after the first, P up to 2^7.97 without a raise, one spiking row in an otherwise flat wave, a common
   offset of +-3000, a first tile 200 below the rest, identical keys.
4. What is NOT written: the output as a view into a canary-filled buffer (row stride C + 8 / C + 64, rows behind Nq, a gap
   between samples, a view 8 bytes off a 16-byte boundary): every canary keeps its bits, the owned elements equal the dense
   call's bit for bit.
5. Argument validation the launcher does on the host; attn_probs / attn_apply_probs at ragged sizes.

MEASURED (MI355X; the digest this module prints when it ends, see `digest` below)
3304 bounded cases; ratio = e_k / e_m, worst of the group; floor = cases the floor alone holds (max / rms)
group                      | cases | max ratio | rms ratio | floor
edges x1.2     bf16 v2     |   189 |      1.98 |      1.17 | 189 / 189
edges x1.2     bf16 v6     |   375 |      1.96 |      1.21 | 375 / 375
edges x1.2     bf16 v7     |   189 |      1.52 |      1.17 | 189 / 189
edges x1.2     fp16 v2     |   189 |      1.78 |      1.43 | 188 / 189
edges x1.2     fp16 v6     |   375 |      1.96 |      1.29 | 373 / 375
edges x1.2     fp16 v7     |   189 |      1.54 |      1.35 | 189 / 189
edges x3.0     bf16 v2     |   189 |      1.14 |      1.17 | 48 / 189
edges x3.0     bf16 v6     |   375 |      1.81 |      1.45 | 131 / 375
edges x3.0     bf16 v7     |   189 |      1.13 |      1.11 | 51 / 189
edges x3.0     fp16 v2     |   189 |      1.63 |      1.20 | 47 / 189
edges x3.0     fp16 v6     |   375 |      2.94 |      1.79 | 134 / 375
edges x3.0     fp16 v7     |   189 |      1.63 |      1.15 | 43 / 189
dominant key   both v2     |    33 |      1.00 |      1.00 | 33 / 33
dominant key   both v6     |   100 |      1.00 |      1.00 | 100 / 100
dominant key   both v7     |    33 |      1.00 |      1.00 | 33 / 33
creep          both all    |    14 |      1.42 |      1.26 | 14 / 14
first-tile-low both all    |    14 |      1.69 |      1.12 | 14 / 14
offset+3000    both all    |    14 |      2.33 |      1.75 | 14 / 14
offset-3000    both all    |    14 |      2.33 |      1.75 | 14 / 14
spike          both all    |    42 |      1.00 |      1.00 | 42 / 42
stairs-down    both all    |    14 |      1.20 |      1.07 | 14 / 14
stairs-up      both all    |    14 |      1.10 |      1.06 | 14 / 14
worst over all cases: max 2.94, rms 1.79; C_MAX = 4, C_RMS = 4
Twice the worst ratios, rounded up to one digit, would be C_MAX = 6 and C_RMS = 4: C_RMS = 4 is that figure; C_MAX stands at the cap of 4
and was NOT raised.  The cases above 2 were looked at: `edge fp16 x3.0 Nkv 128 Nq 1 v6 plain` (2.94) and the bf16 `offset+-3000`
patterns at 128 keys on v6 (2.32).  The first has ONE query row per (sample, head), 256 outputs in all, where the maximum of the
model's error is a noisy yardstick (e_m 5.0e-4 against a floor of 2.5e-3); in all of them the kernel's error is below the floor, one
ulp of the output.  On cases of at least 31 query rows the worst max ratio is 1.98.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from tests import _attn_model as M

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
TOL = {F16: dict(rtol=2e-3, atol=2e-3), BF16: dict(rtol=1.6e-2, atol=1.6e-2)}      # the suite's `close` (tests/test_kernels_gpu.py)

C_MAX = 4.0
C_RMS = 4.0

NKV_CROSS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128]
NQ_CROSS = [1, 33, 130, 513, 640]
NKV_SELF = [129, 130, 191, 192, 193, 255, 257, 320, 1000]
NQ_SELF = [1, 31, 64, 255, 256, 257, 300]
B, HEADS = 2, 2
CC = HEADS * 64


def _name(dtype):
    return "fp16" if dtype == F16 else "bf16"


def _id(v):
    return _name(v) if isinstance(v, torch.dtype) else None


def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


CASES = []          # one record per bounded case: (tag words, max e_k, max e_m, floor, rms e_k, rms e_m, rms floor)
EXACT = {}          # (test, type, kernel) -> worst error of the exact-answer tests, in ulps


def bounded(tag, dtype, out, truth, model_rounded):
    """The module's bound on one case; the case's figures go to CASES (the digest the constants come from) before it asserts."""
    e_k = (out.double().cpu() - truth).abs()
    e_m = (model_rounded - truth).abs()
    floor = M.ulp(dtype) * float(truth.abs().max())
    floor_rms = floor / math.sqrt(12.0)
    mk, mm, rk, rm = float(e_k.max()), float(e_m.max()), M.rms(e_k), M.rms(e_m)
    CASES.append((tag.split(), mk, mm, floor, rk, rm, floor_rms))
    assert bool(torch.isfinite(out).all()), f"{tag}: non-finite output"
    assert mk <= max(floor, C_MAX * mm), f"{tag}: max error {mk:.3e} > max({floor:.3e}, {C_MAX} * {mm:.3e})"
    assert rk <= max(floor_rms, C_RMS * rm), f"{tag}: rms error {rk:.3e} > max({floor_rms:.3e}, {C_RMS} * {rm:.3e})"


def _ratio(a, b):
    return a / b if b > 0 else (1.0 if a == 0 else float("inf"))        # one key: model and kernel both return V's row exactly


@pytest.fixture(scope="module", autouse=True)
def digest():
    yield
    print_digest()


def print_digest():
    """Printed once, after the module's last test (run with -s): the table of the docstring, then per key count the worst case over
    its query counts, kernels and forms (dominant key, stress: per type / pattern).  Tags: `edge <type> x<scale> Nkv n Nq m <kernel> <form>`, `dominant <type> Nkv n <image>
    <kernel>`, `stress <type> Nkv n <pattern> <kernel>`."""
    if not CASES:
        return
    def agg(key):
        groups = {}
        for c in CASES:
            groups.setdefault(key(c[0]), []).append(c)
        for k in sorted(groups):
            g = groups[k]
            wm, wr = max(g, key=lambda c: _ratio(c[1], c[2])), max(g, key=lambda c: _ratio(c[4], c[5]))
            yield k, g, wm, wr
    print(f"\nATTNTABLE {len(CASES)} bounded cases; ratio = e_k / e_m, worst of the group; floor = cases the floor alone holds (max / rms)")
    print(f"ATTNTABLE {'group':26s} | cases | max ratio | rms ratio | floor")
    def table_key(t):
        if t[0] == "edge":
            return ("1 edges " + t[2], t[1], t[7])
        if t[0] == "dominant":
            return ("2 dominant key", "both", t[5])
        return ("3 " + t[4].split("-row")[0], "both", "all")
    for k, g, wm, wr in agg(table_key):
        print(f"ATTNTABLE {k[0][2:]:14s} {k[1]:4s} {k[2]:6s} | {len(g):5d} | {_ratio(wm[1], wm[2]):9.2f} | {_ratio(wr[4], wr[5]):9.2f} | "
              f"{sum(c[1] <= c[3] for c in g)} / {sum(c[4] <= c[6] for c in g)}")
    allm, allr = max(_ratio(c[1], c[2]) for c in CASES), max(_ratio(c[4], c[5]) for c in CASES)
    print(f"ATTNTABLE worst over all cases: max {allm:.2f}, rms {allr:.2f}; C_MAX = {C_MAX:g}, C_RMS = {C_RMS:g}")
    def line_key(t):
        if t[0] == "edge":
            return (0, t[1], t[2], int(t[4]))
        if t[0] == "dominant":
            return (1, t[1], "", 0)
        return (2, t[1], t[4].split("-row")[0], 0)
    for k, g, wm, wr in agg(line_key):
        head = " ".join(wm[0][:5]) if k[0] == 0 else f"{wm[0][0]} {k[1]} {k[2]}".rstrip()
        print(f"ATTNCOND {head} | {len(g)} cases | max {_ratio(wm[1], wm[2]):.2f} at {' '.join(wm[0][5 if k[0] == 0 else 2:])}: e_k {wm[1]:.2e} e_m {wm[2]:.2e} "
              f"floor {wm[3]:.2e} | rms {_ratio(wr[4], wr[5]):.2f} at {' '.join(wr[0][5 if k[0] == 0 else 2:])}: e_k {wr[4]:.2e} e_m {wr[5]:.2e} floor {wr[6]:.2e}")
    for k in sorted(EXACT):
        print(f"ATTNEXACT {' '.join(k)}: worst error {EXACT[k]:.2f} ulp (bound 1)")


class forced_variant:
    """omg_debug_set_attn_variant is process-global: always back to 0."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        L.lib().omg_debug_set_attn_variant(self.v)

    def __exit__(self, *exc):
        L.lib().omg_debug_set_attn_variant(0)


def refs(q, k, v, scale, src=None):
    """truth and the UNROUNDED model of (B, N, heads * 64) CPU tensors, both (B, Nq, heads * 64) float64."""
    qh, kh, vh = M.split_heads(q, HEADS), M.split_heads(k, HEADS), M.split_heads(v, HEADS)
    if src is not None:
        qh, kh = qh[src], kh[src]
    return M.merge_heads(M.truth(qh, kh, vh, scale)), M.merge_heads(M.model(qh, kh, vh, scale))


def run_modes(dev, dtype, tag, q, k, v, scale, nq_list, kernels):
    """Section 1's three forms (plain, borrowed Q / K, accumulate) of one input on each kernel of `kernels`, for every query
    count of `nq_list` (the first rows of q: rows are independent, so one reference serves them all)."""
    src = [0, 0]
    t_plain, m_plain = refs(q, k, v, scale)
    t_src, m_src = refs(q, k, v, scale, src)
    base = randn(B, q.shape[1], CC, seed=11).to(dtype)
    qd, kvd, based = q.to(dev), torch.cat([k, v], dim=2).to(dev), base.to(dev)
    kd, vd = kvd[:, :, :CC], kvd[:, :, CC:]          # strided views of one buffer, as the fused projection leaves them
    srcd = torch.tensor(src, dtype=torch.int32, device=dev)
    operands = {}
    if "v7" in kernels:
        operands["v7"] = ops.value_operand(vd, HEADS)
        assert isinstance(operands["v7"], ops.RowMajorV)
    vt = ops.transpose_v(vd, HEADS)
    for name in kernels:
        if name != "v7":
            operands[name] = vt
    for nq in nq_list:
        outs = {}
        for name in kernels:
            with forced_variant(2 if name == "v2" else 0):
                qs = qd[:, :nq]
                a = ops.attention(qs, kd, operands[name], HEADS, scale)
                b_ = ops.attention(qs, kd, operands[name], HEADS, scale, qk_src=srcd)
                c = based[:, :nq].clone()
                ops.attention(qs, kd, operands[name], HEADS, scale, out=c, accumulate=True, out_scale=0.8)
            outs[name] = (a, b_, c)
        if "v6" in kernels and "v2" in kernels:         # v6 is v2's arithmetic in v2's order
            for x, y in zip(outs["v6"], outs["v2"]):
                assert torch.equal(x, y), f"{tag} Nq {nq}: v6 differs from v2"
        for name in kernels:
            if name == "v2" and "v6" in kernels:
                continue                                # bitwise v6, which is bounded below
            a, b_, c = outs[name]
            t_acc = base[:, :nq].double() + 0.8 * t_plain[:, :nq]
            m_acc = base[:, :nq].double() + 0.8 * m_plain[:, :nq]
            bounded(f"{tag} Nq {nq} {name} plain", dtype, a, t_plain[:, :nq], M.round16(m_plain[:, :nq], dtype))
            bounded(f"{tag} Nq {nq} {name} qk_src", dtype, b_, t_src[:, :nq], M.round16(m_src[:, :nq], dtype))
            bounded(f"{tag} Nq {nq} {name} accumulate", dtype, c, t_acc, M.round16(m_acc, dtype))


def kernels_for(nkv):
    return ("v6", "v2") if nkv <= 128 else ("v7", "v2")


# ------------------------------------------------------------------ 1. every edge
def random_case(dtype, nq, nkv, in_scale):
    q = randn(B, nq, CC, seed=nq + nkv, scale=in_scale).to(dtype)
    k = randn(B, nkv, CC, seed=nkv + 1000, scale=in_scale).to(dtype)
    v = randn(B, nkv, CC, seed=nkv + 2000).to(dtype)
    q[0, 0] = 0                                        # all logits equal
    q[1, 0, :64] = k[1, nkv - 1, :64] * 4              # the LAST real key dominates (head 0)
    return q, k, v


@pytest.mark.parametrize("in_scale", [1.2, 3.0])
@pytest.mark.parametrize("nkv", NKV_CROSS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_cross_attention_edges(dev, dtype, nkv, in_scale):
    q, k, v = random_case(dtype, max(NQ_CROSS), nkv, in_scale)
    run_modes(dev, dtype, f"edge {_name(dtype)} x{in_scale} Nkv {nkv}", q, k, v, 0.125, NQ_CROSS, ("v6", "v2"))


@pytest.mark.parametrize("in_scale", [1.2, 3.0])
@pytest.mark.parametrize("nkv", NKV_SELF)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_self_attention_edges(dev, dtype, nkv, in_scale):
    q, k, v = random_case(dtype, max(NQ_SELF), nkv, in_scale)
    run_modes(dev, dtype, f"edge {_name(dtype)} x{in_scale} Nkv {nkv}", q, k, v, 0.125, NQ_SELF, ("v7", "v2"))


# ------------------------------------------------------------------ 2. exact answers
def one_hot_v(nkv):
    v = torch.zeros(nkv, 64)
    v[torch.arange(nkv), torch.arange(nkv) % 64] = 1
    return v.repeat(1, HEADS).expand(B, nkv, CC)


def tile_index_v(nkv):
    return (torch.arange(nkv) // 64).float()[None, :, None].expand(B, nkv, CC)


def one_ulp_of(exact, dtype):
    """Spacing of the storage type at each element of `exact` (float64, normal range)."""
    _, e = torch.frexp(exact)
    return torch.where(exact == 0, torch.zeros_like(exact), torch.ldexp(torch.ones_like(exact), e - 1)) * M.ulp(dtype)


def run_exact(dev, dtype, tag, q, k, v, scale, exact, nq_list, kernels):
    """Every output within one ulp of the known answer (exact zeros stay zeros), on each kernel."""
    qd, kd, vd = q.to(dev), k.to(dev), v.contiguous().to(dev)
    lim = one_ulp_of(exact, dtype)
    vt = ops.transpose_v(vd, HEADS)
    worst_of = {}
    for nq in nq_list:
        for name in kernels:
            operand = ops.value_operand(vd, HEADS) if name == "v7" else vt
            with forced_variant(2 if name == "v2" else 0):
                out = ops.attention(qd[:, :nq], kd, operand, HEADS, scale)
            err = (out.double().cpu() - exact[:, :nq]).abs()
            worst = float((err / lim[:, :nq].clamp_min(1e-300)).max())
            worst_of[name] = max(worst_of.get(name, 0.0), worst)
            assert bool((err <= lim[:, :nq]).all()), f"{tag} Nq {nq} {name}: {float(err.max()):.3e}, {worst:.2f} ulp"
    for n, w in worst_of.items():
        key = (tag.split()[0], _name(dtype), n)
        EXACT[key] = max(EXACT.get(key, 0.0), w)


@pytest.mark.parametrize("nkv", NKV_CROSS + NKV_SELF)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_uniform_row_is_the_key_count(dev, dtype, nkv):
    """q = 0: a dropped, doubled or phantom key moves a column by 1 / Nkv, a hundred ulps at 1000 keys."""
    nq_list = [1, 130, 513] if nkv <= 128 else [1, 255, 257]
    q = torch.zeros(B, max(nq_list), CC).to(dtype)
    k = randn(B, nkv, CC, seed=nkv, scale=1.5).to(dtype)
    v = one_hot_v(nkv).to(dtype)
    count = torch.bincount(torch.arange(nkv) % 64, minlength=64).double().repeat(HEADS)
    exact = (count / nkv).expand(B, max(nq_list), CC)
    run_exact(dev, dtype, f"uniform {_name(dtype)} Nkv {nkv}", q, k, v, 0.125, exact, nq_list, kernels_for(nkv))


@pytest.mark.parametrize("nkv", NKV_CROSS + NKV_SELF)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_dominant_key_lands_in_its_column(dev, dtype, nkv):
    """Query row j points at key j % Nkv: with Nq >= 64 * ntiles every position of every 16-key group of every tile is the
    dominant one once — the [0-3, 8-11 | 4-7, 12-15] order of transpose_v and of v7's transposing reads position by position,
    the last real key and (v7) the clamped copies behind it."""
    nq = (nkv + 63) // 64 * 64
    k = randn(B, nkv, CC, seed=nkv + 7, scale=1.5).to(dtype)
    q = (k[:, torch.arange(nq) % nkv] * 4).to(dtype)
    images = [("one-hot", one_hot_v(nkv))]
    if nkv <= (2048 if dtype == F16 else 256):          # key // 64 stays exact in the storage type
        images.append(("tile", tile_index_v(nkv)))
    for vname, v in images:
        v = v.to(dtype).contiguous()
        t, m = refs(q, k, v, 0.125)
        want = M.split_heads(v.double(), HEADS)[:, :, torch.arange(nq) % nkv]        # the dominant key's own V row
        assert float((M.split_heads(t, HEADS) - want).abs().max()) < 1e-3 * (1 + float(want.max())), "the construction is not one-hot in float64"
        qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
        vt = ops.transpose_v(vd, HEADS)
        outs = {}
        for name in kernels_for(nkv):
            operand = ops.value_operand(vd, HEADS) if name == "v7" else vt
            with forced_variant(2 if name == "v2" else 0):
                outs[name] = ops.attention(qd, kd, operand, HEADS, 0.125)
        if "v6" in outs:
            assert torch.equal(outs["v6"], outs["v2"])
            del outs["v2"]
        for name, out in outs.items():
            bounded(f"dominant {_name(dtype)} Nkv {nkv} {vname} {name}", dtype, out, t, M.round16(m, dtype))


# ------------------------------------------------------------------ 3. the reference maximum under stress
LN2 = math.log(2.0)
STRESS_NKV = [128, 130, 320, 1024]
STRESS_NQ = 300
PATTERNS = ["stairs-up", "stairs-down", "creep", "spike-row-5", "spike-row-40", "spike-row-290", "offset+3000", "offset-3000", "first-tile-low"]


def stress_case(pattern, dtype, nkv, nq=STRESS_NQ):
    """q = a u + b w, k = c u + n w per head (u: entries +-1/4 on d 0..15, w: on d 16..31; unit, orthogonal): with
    scale = ln 2 the log2-unit logit of (row, key) is exactly a[row] c[key] + b[row] n[key]."""
    g = torch.Generator().manual_seed(nkv + len(pattern))
    rows, keys = torch.arange(nq), torch.arange(nkv)
    tile = (keys // 64).double()
    a, b = torch.ones(nq, dtype=torch.float64), torch.ones(nq, dtype=torch.float64)
    jitter = -((keys % 64) % 5).double() * 0.25        # inside a tile: the maximum (0) at its first key and every fifth after it
    noise = (torch.randn(nkv, generator=g, dtype=torch.float64) * 2.0 * 16).round() / 16
    if pattern == "stairs-up":
        a, c, n = 1 + (rows % 4).double() / 16, 9 * tile, jitter
    elif pattern == "stairs-down":
        a, c, n = 1 + (rows % 4).double() / 16, -9 * tile, jitter
    elif pattern == "creep":
        a, c, n = 1 + (rows % 3).double() / 32, 7.5 * (tile > 0).double(), jitter
    elif pattern.startswith("spike-row-"):
        r = int(pattern.rsplit("-", 1)[1])
        a = (rows == r).double()
        b = torch.zeros(nq, dtype=torch.float64)
        c, n = 20.0 * (keys == nkv - 2).double(), torch.zeros(nkv, dtype=torch.float64)
    elif pattern in ("offset+3000", "offset-3000"):
        a = torch.full((nq,), 50.0 if pattern[6] == "+" else -50.0, dtype=torch.float64)
        c, n = torch.full((nkv,), 60.0, dtype=torch.float64), noise
    elif pattern == "first-tile-low":
        c, n = -200.0 * (tile == 0).double(), noise
    else:
        raise KeyError(pattern)
    q, k = torch.zeros(B, nq, CC, dtype=torch.float64), torch.zeros(B, nkv, CC, dtype=torch.float64)
    for h in range(HEADS):
        sg = torch.where(torch.rand(32, generator=g) < 0.5, -0.25, 0.25).double()
        u, w = sg[:16], sg[16:]
        q[:, :, h * 64: h * 64 + 16] = a[:, None] * u
        q[:, :, h * 64 + 16: h * 64 + 32] = b[:, None] * w
        k[:, :, h * 64: h * 64 + 16] = c[:, None] * u
        k[:, :, h * 64 + 16: h * 64 + 32] = n[:, None] * w
    qs, ks = q.to(dtype), k.to(dtype)
    assert torch.equal(qs.double(), q) and torch.equal(ks.double(), k), "the pattern is not exact in the storage type"
    assert torch.equal(M.scaled_query(qs, LN2), qs), "scale = ln 2 must leave Q' = q"
    v = randn(B, nkv, CC, seed=nkv + 31).to(dtype)
    return qs, ks, v


def assert_shape_of_logits(pattern, q, k, nkv):
    """The achieved float64 log2-unit logits (head 0 of sample 0) have the shape the pattern is named after."""
    s = M.model_logits(q[0, :, :64], k[0, :, :64], LN2)
    ntiles = (nkv + 63) // 64
    tmax = torch.stack([s[:, t * 64: min(nkv, t * 64 + 64)].amax(dim=1) for t in range(ntiles)], dim=1)     # (Nq, ntiles)
    step = tmax[:, 1:] - tmax[:, :-1]
    if pattern == "stairs-up":
        assert bool((step > 8.5).all()) and bool((step < 11).all())          # above ATTN_THR: a raise in every tile
    elif pattern == "stairs-down":
        assert bool((step < -8.5).all())                                     # no raise after tile 0
    elif pattern == "creep":
        assert bool((tmax[:, 0] == 0).all())
        assert bool((tmax[:, 1:] > 7).all()) and bool((tmax[:, 1:] < 8).all())   # below ATTN_THR: never a raise
    elif pattern.startswith("spike-row-"):
        r = int(pattern.rsplit("-", 1)[1])
        others = torch.ones(s.shape[0], dtype=torch.bool)
        others[r] = False
        assert bool((s[others] == 0).all()) and float(s[r, nkv - 2]) == 20.0 and int((s[r] != 0).sum()) == 1
    elif pattern.startswith("offset"):
        off = 3000.0 if pattern[6] == "+" else -3000.0
        assert float((s - off).abs().max()) < 12 and 1.0 < float(s[0].std()) < 3.0
    elif pattern == "first-tile-low":
        assert bool((tmax[:, 0] < tmax[:, 1:].amin(dim=1) - 150).all())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nkv", STRESS_NKV)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_reference_maximum_under_stress(dev, dtype, nkv, pattern):
    q, k, v = stress_case(pattern, dtype, nkv)
    assert_shape_of_logits(pattern, q, k, nkv)
    t, m = refs(q, k, v, LN2)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    vt = ops.transpose_v(vd, HEADS)
    outs = {}
    for name in kernels_for(nkv):
        operand = ops.value_operand(vd, HEADS) if name == "v7" else vt
        with forced_variant(2 if name == "v2" else 0):
            outs[name] = ops.attention(qd, kd, operand, HEADS, LN2)
    if "v6" in outs:
        assert torch.equal(outs["v6"].view(torch.int16), outs["v2"].view(torch.int16))
        del outs["v2"]
    for name, out in outs.items():
        bounded(f"stress {_name(dtype)} Nkv {nkv} {pattern} {name}", dtype, out, t, M.round16(m, dtype))


@pytest.mark.parametrize("nkv", STRESS_NKV)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_identical_keys_give_uniform_probabilities(dev, dtype, nkv):
    """All keys equal: whatever q is, every probability is 1 / Nkv, and with the one-hot V the answer is exact."""
    nq_list = [130, 300]
    q = randn(B, max(nq_list), CC, seed=nkv + 3, scale=1.5).to(dtype)
    k = randn(B, 1, CC, seed=nkv + 4, scale=1.5).to(dtype).expand(B, nkv, CC).contiguous()
    v = one_hot_v(nkv).to(dtype)
    count = torch.bincount(torch.arange(nkv) % 64, minlength=64).double().repeat(HEADS)
    exact = (count / nkv).expand(B, max(nq_list), CC)
    run_exact(dev, dtype, f"identical {_name(dtype)} Nkv {nkv}", q, k, v, 0.125, exact, nq_list, kernels_for(nkv))


# ------------------------------------------------------------------ 4. what is not written
CANARIES = [0x7BFF, 0x7FC1]        # the largest finite fp16 (a large finite bf16); a NaN with a payload in both types
LAYOUTS = {                        # name: (row stride - C, first column of the view, batch gap in rows)
    "ld+8": (8, 0, 0),
    "ld+64": (64, 0, 0),
    "batch-gap": (8, 0, 5),
    "off-8-bytes": (12, 4, 0),     # ldo % 8 == 4, the view starts 8 bytes off a 16-byte boundary: v2's path / v7's 8-byte stores
}


@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kernel,nkv", [("v6", 77), ("v2", 77), ("v2", 130), ("v7", 130)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_nothing_outside_the_output_view_is_written(dev, dtype, kernel, nkv, layout, accumulate):
    """Only memory this test allocated is involved: the view's neighbours are canaries inside the same buffer."""
    pad, col0, gap = LAYOUTS[layout]
    ld = CC + pad
    for canary in CANARIES:
        for nq in [1, 33, 255, 257, 513]:
            q = randn(B, nq, CC, seed=nq, scale=1.2).to(dtype).to(dev)
            kv = randn(B, nkv, 2 * CC, seed=nkv, scale=1.2).to(dtype).to(dev)
            k, v = kv[:, :, :CC], kv[:, :, CC:]
            operand = ops.value_operand(v, HEADS) if kernel == "v7" else ops.transpose_v(v, HEADS)
            base = randn(B, nq, CC, seed=5).to(dtype).to(dev)
            rows = nq + 3 + gap                                         # rows behind Nq, then the gap, all canary
            buf = torch.full((B, rows, ld), canary, dtype=torch.int16, device=dev)
            assert buf.data_ptr() % 16 == 0
            view = buf.view(dtype)[:, :nq, col0: col0 + CC]
            owned = torch.zeros((B, rows, ld), dtype=torch.bool, device=dev)
            owned[:, :nq, col0: col0 + CC] = True
            dense = base.clone() if accumulate else torch.empty(B, nq, CC, dtype=dtype, device=dev)
            if accumulate:
                view.copy_(base)
            kw = dict(accumulate=True, out_scale=0.8) if accumulate else {}
            with forced_variant(2 if kernel == "v2" else 0):
                ops.attention(q, k, operand, HEADS, 0.125, out=dense, **kw)
                ops.attention(q, k, operand, HEADS, 0.125, out=view, **kw)
            torch.cuda.synchronize()
            stray = int((buf[~owned] != canary).sum())
            assert stray == 0, f"{kernel} Nq {nq} Nkv {nkv} {layout} canary {canary:#x}: {stray} elements outside the view were written"
            assert torch.equal(view.contiguous().view(torch.int16), dense.view(torch.int16)), f"{kernel} Nq {nq} Nkv {nkv} {layout}: the view differs from the dense output"


# ------------------------------------------------------------------ 5. small things
def test_attention_refuses_on_the_host_what_it_cannot_run(dev):
    """Every call here is rejected by omg_attn_fwd's argument checks, before anything is launched."""
    q = randn(1, 64, CC + 4, seed=0).half().to(dev)
    kv = randn(1, 256, 2 * CC, seed=1).half().to(dev)
    k, v = kv[:, :, :CC], kv[:, :, CC:]
    vt77, vt256 = ops.transpose_v(v[:, :77], HEADS), ops.transpose_v(v, HEADS)
    good_q = q[:, :, :CC].contiguous()
    with pytest.raises(L.OmgHipError):                                   # ldq % 8 != 0
        ops.attention(q[:, :, :CC], k[:, :77], vt77, HEADS, 0.125)
    with pytest.raises(L.OmgHipError):                                   # ldo % 4 != 0
        ops.attention(good_q, k[:, :77], vt77, HEADS, 0.125, out=torch.empty(1, 64, CC + 2, dtype=torch.float16, device=dev)[:, :, :CC])
    with pytest.raises(L.OmgHipError):                                   # Nkv_pad < Nkv: the image of 64 keys, 77 keys asked for
        ops.attention(good_q, k[:, :77], ops.transpose_v(v[:, :64], HEADS), HEADS, 0.125)
    with pytest.raises(L.OmgHipError):                                   # row-major V with <= 128 keys
        ops.attention(good_q, k[:, :77], ops.RowMajorV(v), HEADS, 0.125)
    with forced_variant(2):
        with pytest.raises(L.OmgHipError):                               # v2 reads a V^T image
            ops.attention(good_q, k, ops.RowMajorV(v), HEADS, 0.125)
    with forced_variant(7):
        with pytest.raises(L.OmgHipError):                               # v7 reads row-major V
            ops.attention(good_q, k, vt256, HEADS, 0.125)
    ops.attention(good_q, k, vt256, HEADS, 0.125)                        # the variant word is back at 0: the same call runs
    torch.cuda.synchronize()


@pytest.mark.parametrize("nq", [1, 5, 130])
@pytest.mark.parametrize("nkv", [1, 63, 64, 65, 77, 130])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_protocol_mode_at_ragged_sizes(dev, dtype, nkv, nq):
    q = randn(B, nq, CC, seed=nq).to(dtype)
    k = randn(B, nkv, CC, seed=nkv + 1).to(dtype)
    v = randn(B, nkv, CC, seed=nkv + 2).to(dtype)
    p = ops.attn_probs(q.to(dev), k.to(dev), HEADS, 0.125)
    pref = M.truth_probs(M.split_heads(q, HEADS), M.split_heads(k, HEADS), 0.125).reshape(B * HEADS, nq, nkv)
    rowsum = p.double().cpu().sum(dim=-1)
    assert float((rowsum - 1).abs().max()) <= nkv * 0.5 * M.ulp(dtype), float((rowsum - 1).abs().max())
    t = TOL[dtype]
    torch.testing.assert_close(p.float().cpu(), pref.float(), rtol=t["rtol"], atol=t["atol"])
    o = ops.attn_apply_probs(p, v.to(dev), HEADS)
    oref = M.merge_heads(p.double().cpu().reshape(B, HEADS, nq, nkv) @ M.split_heads(v, HEADS).double())
    torch.testing.assert_close(o.float().cpu(), oref.float(), rtol=t["rtol"], atol=t["atol"])
