"""LiteMLA's linear attention and depthwise kernels (csrc/litemla.hip: omg_relu_linear_att, omg_dwconv2d, and omg_litemla_aggreg's
depthwise half) at their edges, bounded by a rounding model instead of a fixed tolerance (-m gpu).

References: tests/_litemla_model.py (CPU, on the STORED 16-bit operands).  tests/test_litemla_model.py shows without a GPU that the
checks below reject a kernel with any one of nine faults.

1. Linear attention against `truth` (float64) under the rule, elementwise, no element excluded:

       |out[i] - truth[i]|  <=  ulp16(truth[i]) / 2  +  C * E32,      out finite

   E32 = max |ref32 - truth| over the case (torch's fp32 evaluation of the same formula), floored at 2^-23 max |truth|; C = 4 (C_MAX of
   tests/test_attention_conditioning_gpu.py).  HW in {1, 63, 65, 127, 128, 129, 255, 257, 300} x dim in {8, 16, 32} (one token, one
   128-token chunk exactly, one token either side of 64 / 128 / 256 tokens per block), (B, G) in {(1, 1), (2, 3)}, and the real shape
   (1, 4096, 2, 32); families plain, sparse_offset (dead query rows), cancel, wide; eps in {1e-15, 0.5, 8.0}.  EVERY call of this module
   reads a column slice of a wider buffer, writes through out= into a canary frame (canary columns on both sides, a canary row behind
   the last token) and gets a NaN-filled workspace with canary floats behind omg_relu_linear_att_ws_floats: every canary keeps its
   bits, every workspace float is written, the result is finite.
2. Exact answers (torch.equal): residue classes (k_t = e_(t mod dim), q_t = 2 e_((7 t + 3) mod dim), integer v: the mean of v over
   a residue class of the token's own sample and group); a query without a positive channel; a group whose k is never positive.
3. Bitwise invariances: q x 4, k x 4 (no bit changes), v x 4 (4 x the output), a sample alone against the same sample between two
   samples of 1000s, a permutation of the groups.
4. omg_dwconv2d bit for bit against `dwconv_emulation`: k in {1, 3, 5, 7, 9} x (H, W) in {(1, 1), (1, 5), (3, 2), (8, 8), (13, 7)} x
   C in {8, 24, 200}, B = 2, with and without bias, column-slice input, canary-framed out=; the middle image of a batch of three.
5. omg_litemla_aggreg with a per-group identity weight equals omg_dwconv2d bit for bit ("the same value omg_dwconv2d would
   have stored"), k in {1, 3, 5, 7, 9}.

MEASURED (MI355X; the digest this module prints when it ends; with OMG_LITEMLA_ERRORS_JSON=path every case's figures go to that file)
A 16-bit output does not show the kernel's fp32 value, so "kernel error over E32" is measured from below: `excess` is the error beyond
the half ulp of the one rounding to the storage type, which the fp32 value must have had at least.  On the CPU emulation of the
kernel's summation order (tests/test_litemla_model.py, where the fp32 value is visible) the fp32 error over E32 is at most 1.45.
476 cases of the rule; worst of each group
group          type | cases | excess / E32 | error / bound | not round16(truth)
dead           bf16 |     3 |         0.02 |          1.00 | 0.0002
dead           fp16 |     3 |         0.08 |          0.99 | 0.0002
edge           bf16 |   216 |         0.42 |          1.00 | 0.0010
edge           fp16 |   216 |         0.62 |          1.00 | 0.0107
eps0.5         bf16 |     6 |         0.09 |          1.00 | 0.0001
eps0.5         fp16 |     6 |         0.56 |          1.00 | 0.0006
eps1e-15       bf16 |     6 |         0.07 |          1.00 | 0.0000
eps1e-15       fp16 |     6 |         0.21 |          1.00 | 0.0006
eps8.0         bf16 |     6 |         0.13 |          1.00 | 0.0001
eps8.0         fp16 |     6 |         0.17 |          1.00 | 0.0008
real           bf16 |     1 |         0.06 |          1.00 | 0.0001
real           fp16 |     1 |         0.31 |          1.00 | 0.0004
worst over all cases: excess / E32 0.62, error / bound 1.00, not round16(truth) 0.0107; C = 4.0
The error reaches the bound only where it is the half ulp of the one rounding (error / bound 1.00 with an excess of 0.62 E32 of the 4 E32
granted, on `edge sparse_offset B2 HW300 G3 dim32` fp16): C was not raised and has room.  The shares above 0.2 % are all `cancel`
cases of one sample and one group (1.07 % on HW 129 dim 8 fp16: 11 of 1032 elements), where kv cancels and E32 is large against the
output's ulp; everywhere else at most 0.2 % of the elements differ from round16(truth).  The exact, bitwise, depthwise and aggregation
tests (sections 2 - 5) passed as written: no kernel fault was found.
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from tests import _litemla_model as M

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
HWS = [1, 63, 65, 127, 128, 129, 255, 257, 300]
DIMS = [8, 16, 32]
BGS = [(1, 1), (2, 3)]
CANARY = -1234.0                # exact in fp16, -1232 in bf16: the frame is compared with itself, bit for bit
WS_CANARY = 54321.0

CASES = []                      # one record per case of the rule (M.held)


def _id(v):
    return M.name(v) if isinstance(v, torch.dtype) else None


@pytest.fixture(scope="module", autouse=True)
def digest():
    yield
    print_digest()


def print_digest():
    if not CASES:
        return
    groups = {}
    for c in CASES:
        groups.setdefault((c["tag"].split()[0], c["dtype"]), []).append(c)
    print(f"\n{len(CASES)} cases of the rule; worst of each group")
    print("group          type | cases | excess / E32 | error / bound | not round16(truth)")
    for key in sorted(groups):
        g = groups[key]
        print(f"{key[0]:14s} {key[1]} | {len(g):5d} | {max(c['excess_over_E32'] for c in g):12.2f} | {max(c['err_over_bound'] for c in g):13.2f} | "
              f"{max(c['not_round_truth'] for c in g):.4f}")
    print(f"worst over all cases: excess / E32 {max(c['excess_over_E32'] for c in CASES):.2f}, error / bound {max(c['err_over_bound'] for c in CASES):.2f}, "
          f"not round16(truth) {max(c['not_round_truth'] for c in CASES):.4f}; C = {M.C_RULE}")
    path = os.environ.get("OMG_LITEMLA_ERRORS_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(CASES, f, indent=1)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def framed(rows, cols, dtype, dev):
    """A canary frame [rows + 1, cols + 16] and the view [rows, cols] inside it at column 8 (16-byte aligned)."""
    frame = torch.full((rows + 1, cols + 16), CANARY, dtype=dtype, device=dev)
    return frame, frame[:rows, 8:8 + cols]


def frame_untouched(frame, rows, cols):
    after = frame.clone()
    after[:rows, 8:8 + cols] = CANARY
    return torch.equal(bits(after), bits(torch.full_like(frame, CANARY)))


def sliced(t, dev, fill=77.0):
    """`t` [rows, cols] as a column slice (at column 8) of a wider device buffer whose other columns hold `fill`."""
    wide = torch.full((t.shape[0], t.shape[1] + 24), fill, dtype=t.dtype)
    wide[:, 8:8 + t.shape[1]] = t
    return wide.to(dev)[:, 8:8 + t.shape[1]]


def rla(dev, qkv, B, HW, G, dim, eps):
    """ops.relu_linear_att with everything guarded; returns the output on the CPU."""
    rows = B * HW
    frame, view = framed(rows, G * dim, qkv.dtype, dev)
    need = int(L.lib().omg_relu_linear_att_ws_floats(B, G, dim, HW))
    assert need == B * G * ((HW + 127) // 128) * dim * (dim + 1)
    ws = torch.full((need + 64,), float("nan"), dtype=torch.float32, device=dev)
    ws[need:] = WS_CANARY
    x = sliced(qkv, dev)
    assert x.stride(0) > G * 3 * dim and view.stride(0) > G * dim
    out = ops.relu_linear_att(x, B, HW, G, dim, eps, out=view, workspace=ws)
    assert out.data_ptr() == view.data_ptr()
    assert frame_untouched(frame, rows, G * dim), "wrote outside its column slice or behind the last token"
    assert torch.equal(bits(ws[need:]), bits(torch.full((64,), WS_CANARY, device=dev))), "wrote behind omg_relu_linear_att_ws_floats"
    assert not bool(torch.isnan(ws[:need]).any()), "a workspace float was never written"
    out = out.cpu().contiguous()
    assert bool(torch.isfinite(out).all()), "non-finite output: a partial sum was read that nobody wrote"
    dense = ops.relu_linear_att(x, B, HW, G, dim, eps)                     # the default path: own output, own workspace
    assert torch.equal(bits(dense.cpu()), bits(out))
    return out


def ruled(dev, tag, qkv, B, HW, G, dim, eps):
    out = rla(dev, qkv, B, HW, G, dim, eps)
    M.held(tag, qkv.dtype, out, M.truth(qkv, B, HW, G, dim, eps), M.ref32(qkv, B, HW, G, dim, eps), log=CASES)
    return out


# ------------------------------------------------------------------------------------------------------------- 1. the rule at every edge
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", M.FAMILIES)
def test_relu_linear_att_holds_the_rule_at_every_edge(dev, dtype, dim, kind):
    for B, G in BGS:
        for HW in HWS:
            qkv = M.family(kind, B, HW, G, dim, seed=1000 * dim + HW + G).to(dtype)
            if kind == "sparse_offset" and B * HW * G >= 120:                 # enough rows for a share to mean something
                dead, live = M.dead_and_live_rows(qkv, B, HW, G, dim)
                assert dead >= 0.05 and live >= 0.25, (B, HW, G, dim, dead, live)
            ruled(dev, f"edge {kind} B{B} HW{HW} G{G} dim{dim}", qkv, B, HW, G, dim, 1e-15)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_relu_linear_att_holds_the_rule_at_the_real_shape(dev, dtype):
    B, HW, G, dim = 1, 4096, 2, 32                                            # 32 chunks, 64 token blocks
    ruled(dev, f"real plain B{B} HW{HW} G{G} dim{dim}", M.family("plain", B, HW, G, dim, seed=4096).to(dtype), B, HW, G, dim, 1e-15)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("eps", [1e-15, 0.5, 8.0])
def test_relu_linear_att_adds_eps_to_the_denominator(dev, dtype, dim, eps):
    B, HW, G = 2, 129, 3
    for kind in ("plain", "sparse_offset"):
        qkv = M.family(kind, B, HW, G, dim, seed=50 + dim).to(dtype)
        out = ruled(dev, f"eps{eps} {kind} B{B} HW{HW} G{G} dim{dim}", qkv, B, HW, G, dim, eps)
        if eps >= 0.5:                                                        # the case can tell: against the answer without eps it breaks the rule
            with pytest.raises(AssertionError):
                M.held("no eps", dtype, out, M.truth(qkv, B, HW, G, dim, 1e-15), M.ref32(qkv, B, HW, G, dim, 1e-15))


# --------------------------------------------------------------------------------------------------------------------- 2. exact answers
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("dim", DIMS)
def test_relu_linear_att_residue_classes_are_exact(dev, dtype, dim):
    B, HW, G = 2, 256, 3
    g = torch.Generator().manual_seed(2)
    x = torch.zeros(B, HW, G, 3 * dim)
    t = torch.arange(HW)
    x[:, t, :, dim + t % dim] = 1.0                                            # k_t = e_(t mod dim)
    x[:, t, :, (7 * t + 3) % dim] = 2.0                                        # q_t = 2 e_((7 t + 3) mod dim)
    x[..., 2 * dim:] = torch.randint(-8, 9, (B, HW, G, dim), generator=g).float()
    cls = x[..., 2 * dim:].permute(0, 2, 1, 3).reshape(B, G, HW // dim, dim, dim).mean(2)           # [B, G, residue, dim]
    want = cls[:, :, (7 * t + 3) % dim].permute(0, 2, 1, 3).reshape(B * HW, G * dim)
    assert torch.equal(want, want.to(dtype).float()), "the case itself must be exactly representable"
    w = want.reshape(B, HW, G, dim)
    assert not torch.equal(w[0], w[1]) and not torch.equal(w[:, :, 0], w[:, :, 1]) and not torch.equal(w[:, :, 1], w[:, :, 2])
    out = rla(dev, x.reshape(B * HW, -1).to(dtype), B, HW, G, dim, 1e-15)
    assert torch.equal(out.float(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("dim", DIMS)
def test_relu_linear_att_dead_queries_and_dead_groups_return_exact_zeros(dev, dtype, dim):
    B, HW, G = 2, 130, 3
    x = M.family("plain", B, HW, G, dim, seed=60 + dim).reshape(B * HW, G, 3 * dim)
    dead_rows = torch.arange(0, B * HW, 7)
    x[dead_rows, :, :dim] = -x[dead_rows, :, :dim].abs()                       # no positive channel in q ...
    x[dead_rows[::2], :, :dim] = 0.0                                           # ... or all zero
    x[:, 1, dim:2 * dim] = -x[:, 1, dim:2 * dim].abs()                         # group 1: k never positive
    x[::3, 1, dim:2 * dim] = 0.0
    qkv = x.reshape(B * HW, -1).to(dtype)
    out = ruled(dev, f"dead plain B{B} HW{HW} G{G} dim{dim}", qkv, B, HW, G, dim, 1e-15).reshape(B * HW, G, dim)      # the neighbours hold the rule
    zero = torch.zeros((), dtype=dtype)
    assert torch.equal(out[dead_rows], zero.expand(len(dead_rows), G, dim))
    assert torch.equal(out[:, 1], zero.expand(B * HW, dim))
    alive = (qkv.reshape(B * HW, G, 3 * dim)[..., :dim] > 0).any(-1)           # every query with a positive channel, and no other
    alive[:, 1] = False
    assert torch.equal(out.abs().amax(-1) > 0, alive) and int(alive.sum()) > B * HW


# ---------------------------------------------------------------------------------------------------------------- 3. bitwise invariances
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("dim", DIMS)
def test_relu_linear_att_power_of_two_scalings_are_bitwise(dev, dtype, dim):
    """eps = 1e-15 is below half an ulp of every non-zero fp32 denominator here (and a zero one returns 0 either way), so 4 q and 4 k
    scale numerator and denominator alike; 4 v scales the numerator.  The seed is the one tests/test_litemla_model.py checks on the
    emulation."""
    B, HW, G = 2, 129, 3
    qkv = M.family("plain", B, HW, G, dim, seed=21).to(dtype)
    base = rla(dev, qkv, B, HW, G, dim, 1e-15)
    for part in range(3):
        s = qkv.clone().reshape(B * HW, G, 3, dim)
        s[:, :, part] *= 4
        got = rla(dev, s.reshape(B * HW, -1), B, HW, G, dim, 1e-15)
        if part < 2:
            assert torch.equal(bits(got), bits(base)), "qk"[part]
        else:
            normal = base.float().abs() >= (2.0 ** -14 if dtype == F16 else 2.0 ** -126)       # 4 round(x) is round(4 x) unless x is subnormal
            assert float(normal.float().mean()) > 0.99
            assert torch.equal(got.float()[normal], 4 * base.float()[normal])
            assert bool(((got.float() - 4 * base.float()).abs()[~normal] <= 4 * 2.0 ** -24).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("dim", DIMS)
def test_relu_linear_att_sample_and_group_invariance(dev, dtype, dim):
    HW, G = 129, 3
    one = M.family("plain", 1, HW, G, dim, seed=21).to(dtype)
    alone = rla(dev, one, 1, HW, G, dim, 1e-15)
    big = torch.full_like(one, 1000.0)
    three = rla(dev, torch.cat([big, one, -big]), 3, HW, G, dim, 1e-15)
    assert torch.equal(bits(three[HW:2 * HW]), bits(alone))
    perm = [2, 0, 1]
    moved = one.reshape(HW, G, 3 * dim)[:, perm].reshape(HW, -1).contiguous()
    got = rla(dev, moved, 1, HW, G, dim, 1e-15)
    assert torch.equal(bits(got), bits(alone.reshape(HW, G, dim)[:, perm].reshape(HW, -1)))


# ------------------------------------------------------------------------------------------------------------ 4. depthwise, bit for bit
def dw(dev, x, taps, bias, B, H, W, k):
    rows, C = x.shape
    frame, view = framed(rows, C, x.dtype, dev)
    out = ops.dwconv2d(sliced(x, dev), taps.to(dev), B, H, W, k, bias=None if bias is None else bias.to(dev), out=view)
    assert out.data_ptr() == view.data_ptr()
    assert frame_untouched(frame, rows, C), "wrote outside its column slice or behind the last pixel"
    return out.cpu().contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("k", [1, 3, 5, 7, 9])
def test_dwconv2d_equals_its_emulation_bit_for_bit(dev, dtype, k):
    B = 2
    for H, W in [(1, 1), (1, 5), (3, 2), (8, 8), (13, 7)]:
        for C in (8, 24, 200):
            x, taps, bias = M.dwconv_inputs(B, H, W, C, k, dtype, seed=100 * k + H + W + C)
            for b in (bias, None):
                got = dw(dev, x, taps, b, B, H, W, k)
                want = M.dwconv_emulation(x, taps, b, B, H, W, k).to(dtype)
                same = bits(got) == bits(want)
                assert bool(same.all()), (f"k{k} {H}x{W} C{C} bias {b is not None}: {int((~same).sum())} of {same.numel()} differ, "
                                          f"max |d| {float((got.float() - want.float()).abs().max()):.3e}")
            dense = ops.dwconv2d(sliced(x, dev), taps.to(dev), B, H, W, k, bias=bias.to(dev))      # the default path: its own output
            assert torch.equal(bits(dense.cpu()), bits(dw(dev, x, taps, bias, B, H, W, k)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("k", [3, 9])
def test_dwconv2d_taps_stay_inside_their_image(dev, dtype, k):
    for H, W in [(3, 2), (8, 8)]:
        C = 24
        x, taps, bias = M.dwconv_inputs(1, H, W, C, k, dtype, seed=7)
        big = torch.full_like(x, 1000.0)
        alone = dw(dev, x, taps, bias, 1, H, W, k)
        three = dw(dev, torch.cat([big, x, -big]), taps, bias, 3, H, W, k)
        assert torch.equal(bits(three[H * W:2 * H * W]), bits(alone))
        assert torch.equal(bits(alone), bits(M.dwconv_emulation(x, taps, bias, 1, H, W, k).to(dtype)))


# ---------------------------------------------------------------------------------------- 5. the fused aggregation's depthwise half
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("dim", [16, 32])
@pytest.mark.parametrize("k", [1, 3, 5, 7, 9])
def test_litemla_aggreg_with_identity_groups_is_dwconv2d(dev, dtype, dim, k):
    """Wg[g dim + o][i] = [o == i]: the MFMA adds exact zeros to 1 * round16(depthwise), so the fused kernel must store what
    omg_dwconv2d stores.  3 dim channels: one and a half / three tiles of 32; 9 dim: more than one block of four waves."""
    B = 2
    for H, W in [(3, 2), (13, 7)]:
        for C in (3 * dim, 9 * dim):
            x, taps, _ = M.dwconv_inputs(B, H, W, C, k, dtype, seed=200 * k + H + C, with_bias=False)
            wg = torch.eye(dim, dtype=dtype).repeat(C // dim, 1)
            frame, view = framed(B * H * W, C, dtype, dev)
            got = ops.litemla_aggreg(sliced(x, dev), taps.to(dev), wg.to(dev), B, H, W, k, dim, out=view)
            assert frame_untouched(frame, B * H * W, C)
            want = dw(dev, x, taps, None, B, H, W, k)
            assert torch.equal(bits(got.cpu()), bits(want)), (k, H, W, C)
            assert torch.equal(bits(want), bits(M.dwconv_emulation(x, taps, None, B, H, W, k).to(dtype)))
