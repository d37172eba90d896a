"""The four producers of the MX-fp8 operand format (-m gpu) against oracle/mx8.py, byte for byte, on CONSTRUCTED inputs
(tests/_mx8_patterns.py; the oracle itself is checked against its contract in tests/test_oracle_mx8.py):

a. omg_quant_mx8 on every element: per binade of the input type an amax of mantissa 1.0 / 1.75 / 1.75 -+ 1 ulp / all ones, and
   under each every input pattern within 2^-14 of it, the e4m3 subnormal grid with its ties, +-0 and underflowing values — ties to
   even, subnormals, underflow and the sign of an underflowed negative are forced, not left to randn.  The bf16 amax range
   9.2e-41 .. 448 * 2^-126, where an fp32 subnormal inside the scale rule would show, has a test of its own.
b. non-finite input: the three sentences of the contract in oracle/mx8.py.
c. layout of omg_quant_mx8: rows off the 32-row workgroup, strided x / q / scales, canaries around everything, refusals.
d. omg_layernorm_mx8 / omg_groupnorm_mx8 on chosen values: gamma = 0 and beta = p make the normalised value exactly p, so the
   fused kernels quantise the patterns of (a); expected = the oracle applied to the 16-bit kernel's own output, which must
   equal beta up to the sign of zero.  Every vector count per lane, ragged vector groups, the three scale-store forms of
   GroupNorm with and without pad channels, a concat boundary inside a block, two vectors per lane (C = 2560).
(e. the GEGLU epilogue's fp8 output shares the helpers; its layout case lives next to its test in tests/test_mx8_gpu.py.)

Nothing here has a tolerance.  A failure prints the first offending input pattern with the expected and the received byte.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from oracle import mx8
from tests import _mx8_patterns as P

DTYPES = [torch.float16, torch.bfloat16]
CANARY = 0xA5
CANARY32 = -1515870811                                   # 0xA5A5A5A5 as int32
OMG_EINVAL = -1                                          # include/omg_hip.h


def _assert_matches_oracle(x, got_q, got_scales, what=""):
    """x [M, K] 16-bit on the CPU; got_q uint8 [M, K], got_scales int32 [K/128, >= M] (CPU)."""
    M = x.shape[0]
    q, packed, ex = mx8.quantize(x.float())
    if torch.equal(got_q, q) and torch.equal(got_scales[:, :M], packed):
        return
    pytest.fail(what + "\n" + P.describe_first_mismatch(x, got_q, q, P.scale_bytes(got_scales, M), (ex + 127).to(torch.int64)))


# ---- a. every element ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_under_every_amax(dev, dtype):
    x = P.every_element_sweep(dtype)
    got = ops.quant_mx8(x.to(dev))
    _assert_matches_oracle(x, got.q.cpu(), got.scales.cpu())


def test_tiny_bf16_amax_scale_byte(dev):
    """amax from 9.2e-41 to 448 * 2^-126: amax / 448 is an fp32 subnormal, the contract still holds — byte 0 up to
    448 * 2^-127 (the clamp), byte 1 above."""
    x = P.tiny_bf16_sweep()
    got = ops.quant_mx8(x.to(dev))
    _assert_matches_oracle(x, got.q.cpu(), got.scales.cpu())


# ---- b. non-finite input ------------------------------------------------------------------------------------------
def _non_finite_cases(dtype):
    """[3 * cases, 256]: per case a row of finite data, the affected row, another finite row.  The affected block is block
    `blk` of stage `stage`; the bad element sits first / last / on either side of the lane boundary, or alone among zeros."""
    g = torch.Generator().manual_seed(17)
    rows, where = [], []
    for bad in (float("inf"), float("-inf"), float("nan")):
        for pos in (0, 31, 15, 16, "alone"):
            for blk in range(4):
                stage = (blk + len(where)) % 2
                r = torch.randn((3, 256), generator=g)
                c0 = stage * 128 + blk * 32
                if pos == "alone":
                    r[1, c0:c0 + 32] = 0
                r[1, c0 + (7 if pos == "alone" else pos)] = bad
                rows.append(r)
                where.append((len(where) * 3 + 1, c0 // 32))
    return torch.cat(rows).to(dtype), where


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_input_stays_nan_and_stays_in_its_block(dev, dtype):
    x, where = _non_finite_cases(dtype)
    M = x.shape[0]
    got = ops.quant_mx8(x.to(dev))
    gq, gb = got.q.cpu(), P.scale_bytes(got.scales.cpu(), M)
    q, _, ex, unspec = mx8.quantize(x.float(), return_unspecified=True)
    assert int(unspec.sum()) == len(where) and all(bool(unspec[r, b]) for r, b in where)
    bad = ~torch.isfinite(x.float())
    nan_byte = (gq[bad] & 0x7f) == 0x7f
    assert nan_byte.all(), f"a non-finite element was stored as byte 0x{int(gq[bad][~nan_byte][0]):02x}, not as an e4m3 NaN"
    want_b = (ex + 127).to(torch.int64)
    keep = ~unspec.repeat_interleave(32, dim=1)
    if not (torch.equal(gq[keep], q[keep]) and torch.equal(gb[~unspec], want_b[~unspec])):
        pytest.fail("a block without a non-finite element changed\n" + P.describe_first_mismatch(x, gq, q, gb, want_b, skip=unspec))


# ---- c. layout ----------------------------------------------------------------------------------------------------
def _strided_operands(dev, dtype, M, K, seed):
    """x as a column-offset view (ldx = K + 8); q (ldq = K + 16) and the scale array (s_ld = M rounded up to 4, plus 4) inside
    canary-filled buffers with a guard row before and after."""
    g = torch.Generator().manual_seed(seed)
    xb = (torch.randn((M, K + 8), generator=g) * 4).to(dtype).to(dev)
    s_ld = (M + 3) // 4 * 4 + 4
    qb = torch.full((M + 2, K + 16), CANARY, dtype=torch.uint8, device=dev)
    sb = torch.full((K // 128 + 2, s_ld), CANARY32, dtype=torch.int32, device=dev)
    return xb, xb[:, 8:], qb, qb[1:M + 1], sb, sb[1:-1]


def _assert_canaries(qb, sb, M, K):
    qc, sc = qb.cpu().clone(), sb.cpu().clone()
    qc[1:M + 1, :K] = CANARY
    sc[1:-1, :M] = CANARY32
    assert (qc == CANARY).all(), "bytes outside q[M, K] were written"
    assert (sc == CANARY32).all(), "dwords outside scales[K/128, M] were written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 65])
def test_quantiser_strided_operands_and_canaries(dev, dtype, M, K):
    xb, x, qb, q, sb, s = _strided_operands(dev, dtype, M, K, seed=100 + M + K)
    assert x.stride(0) == K + 8 and q.stride(0) == K + 16 and s.stride(0) == (M + 3) // 4 * 4 + 4 and x.data_ptr() == xb.data_ptr() + 16
    rc = L.lib().omg_quant_mx8(ops._dt(x), x.data_ptr(), x.stride(0), M, K, q.data_ptr(), q.stride(0), s.data_ptr(), s.stride(0), ops._stream())
    L.check(rc, "omg_quant_mx8")
    _assert_matches_oracle(x.cpu().contiguous(), q[:, :K].cpu().contiguous(), s.cpu())
    _assert_canaries(qb, sb, M, K)


@pytest.mark.parametrize("why", ["K % 128", "ldx % 8", "ldq % 16", "s_ld < M", "s_ld % 4", "null x", "null q", "null scales"])
def test_quantiser_refuses_and_writes_nothing(dev, why):
    M, K = 33, 256
    xb, x, qb, q, sb, s = _strided_operands(dev, torch.float16, M, K, seed=7)
    a = dict(x=x.data_ptr(), ldx=x.stride(0), K=K, q=q.data_ptr(), ldq=q.stride(0), s=s.data_ptr(), s_ld=s.stride(0))
    a.update({"K % 128": dict(K=K - 64), "ldx % 8": dict(ldx=K + 4), "ldq % 16": dict(ldq=K + 8), "s_ld < M": dict(s_ld=32), "s_ld % 4": dict(s_ld=38),
              "null x": dict(x=None), "null q": dict(q=None), "null scales": dict(s=None)}[why])
    rc = L.lib().omg_quant_mx8(L.OMG_F16, a["x"], a["ldx"], M, a["K"], a["q"], a["ldq"], a["s"], a["s_ld"], ops._stream())
    torch.cuda.synchronize()
    assert rc == OMG_EINVAL
    assert (qb == CANARY).all() and (sb == CANARY32).all()


# ---- d. the fused producers on chosen values ------------------------------------------------------------------------
def _beta(dtype, C, seed):
    return P.to_tensor(P.chosen_blocks(dtype, C // 32, seed), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 5, 77])
@pytest.mark.parametrize("C", [128, 640, 1152, 2048])
def test_layernorm_mx8_on_chosen_values(dev, dtype, C, M):
    lib = L.lib()
    beta = _beta(dtype, C, seed=C + M)
    g = torch.Generator().manual_seed(C * 100 + M)
    xb = (torch.randn((M, C + 8), generator=g) * 3).to(dtype).to(dev)
    x = xb[:, 8:]                                            # ldx = C + 8
    gamma, beta_d = torch.zeros(C, dtype=dtype, device=dev), beta.to(dev)
    y16 = torch.empty((M, C), dtype=dtype, device=dev)
    L.check(lib.omg_layernorm(ops._dt(x), x.data_ptr(), x.stride(0), M, C, 1e-5, gamma.data_ptr(), beta_d.data_ptr(), y16.data_ptr(), y16.stride(0),
                              ops._stream()), "omg_layernorm")
    s_ld = (M + 3) // 4 * 4 + 4
    qb = torch.full((M + 2, C + 16), CANARY, dtype=torch.uint8, device=dev)
    sb = torch.full((C // 128 + 2, s_ld), CANARY32, dtype=torch.int32, device=dev)
    q, s = qb[1:M + 1], sb[1:-1]
    L.check(lib.omg_layernorm_mx8(ops._dt(x), x.data_ptr(), x.stride(0), M, C, 1e-5, gamma.data_ptr(), beta_d.data_ptr(), q.data_ptr(), q.stride(0),
                                  s.data_ptr(), s.stride(0), ops._stream()), "omg_layernorm_mx8")
    y = y16.cpu()
    bad = y.float() != beta.float()[None, :]                 # -0 == +0: equal up to the sign of zero
    assert not bad.any(), f"omg_layernorm with gamma = 0 is not beta: channel {int(bad.nonzero()[0][1])}, beta pattern 0x{int(beta.view(torch.int16)[int(bad.nonzero()[0][1])]) & 0xffff:04x}"
    _assert_matches_oracle(y, q[:, :C].cpu().contiguous(), s.cpu())
    _assert_canaries(qb, sb, M, C)


GN_CASES = [(32, 0), (96, 0), (64, 0), (320, 0), (128, 0), (640, 0),      # per-block / per-64 / per-128 scale stores, each with pad channels or without
            (40, 24), (72, 56),                                            # a concat boundary inside a 32-channel block
            (2560, 0)]                                                     # two channel vectors per lane
GUARD = 256


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C1,C2", GN_CASES)
def test_groupnorm_mx8_on_chosen_values(dev, dtype, C1, C2):
    lib = L.lib()
    C = C1 + C2
    Cq = (C + 127) // 128 * 128
    groups = min(32, C // 8)
    beta = _beta(dtype, C, seed=C1 + 3 * C2)
    gamma, beta_d = torch.zeros(C, dtype=dtype, device=dev), beta.to(dev)
    for HW in (1, 7, 300):                                   # a single pixel, fewer pixels than pixel rows, ragged chunks
        for B in (1, 3):
            g = torch.Generator().manual_seed(HW * 10 + B)
            x1 = (torch.randn((B, HW, C1), generator=g) * 2 + 0.5).to(dtype).to(dev)
            x2 = (torch.randn((B, HW, C2), generator=g) * 5).to(dtype).to(dev) if C2 else None
            y = ops.groupnorm(x1, gamma, beta_d, groups, 1e-5, silu=False, x2=x2).cpu().reshape(B * HW, C)
            bad = y.float() != beta.float()[None, :]
            assert not bad.any(), f"omg_groupnorm with gamma = 0 is not beta: HW {HW}, B {B}, channel {int(bad.nonzero()[0][1])}"
            P_ = B * HW
            qb = torch.full((GUARD + P_ * Cq + GUARD,), CANARY, dtype=torch.uint8, device=dev)
            sb = torch.full((GUARD + Cq // 128 * P_ + GUARD,), CANARY32, dtype=torch.int32, device=dev)
            q, s = qb[GUARD:GUARD + P_ * Cq].view(P_, Cq), sb[GUARD:GUARD + Cq // 128 * P_].view(Cq // 128, P_)
            ws = ops._gn_workspace(dev, B, groups, HW)
            L.check(lib.omg_groupnorm_mx8(ops._dt(x1), x1.data_ptr(), C1, ops._p(x2), C2, B, HW, groups, 1e-5, gamma.data_ptr(), beta_d.data_ptr(), 0,
                                          ws.data_ptr(), q.data_ptr(), s.data_ptr(), ops._stream()), "omg_groupnorm_mx8")
            yp = torch.zeros((P_, Cq), dtype=dtype)          # pad channels: zero bytes, scale byte 0
            yp[:, :C] = y
            _assert_matches_oracle(yp, q.cpu(), s.cpu(), what=f"HW {HW}, B {B}")
            assert (qb[:GUARD] == CANARY).all() and (qb[-GUARD:] == CANARY).all(), f"HW {HW}, B {B}: bytes outside Q were written"
            assert (sb[:GUARD] == CANARY32).all() and (sb[-GUARD:] == CANARY32).all(), f"HW {HW}, B {B}: dwords outside the scale array were written"
