"""omg_attn_swin, omg_swin_merge_ln and omg_swin_patch_embed (csrc/swin.hip) against literal torch compositions in float64 (-m gpu).

Attention.  The reference is tests/swin_torch.py::attention_from_qkv on the STORED 16-bit inputs in float64: pad, roll, partition,
table bias, -100 region mask, softmax, reverse, roll back, crop.  The bound is the rule of tests/test_attention_conditioning_gpu.py,
with its constants: with `truth` that reference, `model` the same with the design's rounding points only (exact scores on the 16-bit
operands, P = round16(exp(S - rowmax)), O = P v / sum P on the unrounded sum, rounded once to the storage type), e_k = |kernel - truth|
and e_m = |model - truth| over the whole output of a case,

    max(e_k) <= max(FLOOR, C_MAX * max(e_m))   and   rms(e_k) <= max(FLOOR_RMS, C_RMS * rms(e_m)),   C_MAX = C_RMS = 4,

FLOOR = one ulp of the storage type at the case's largest |truth|, FLOOR_RMS = FLOOR / sqrt(12).  Inputs: q and k at a scale that
spreads the scores over several units, a table of +- 1.5: the softmax rows are far from uniform, so a wrong mask, shift or bias index
is tens of per cent, not a rounding.

Merge + LayerNorm and the patch rows are held to the norm tests' rule (tests/test_norm_conditioning_gpu.py: `close` with scale 2); the
patch rows themselves are a gather and must be exact.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from tests import _attn_model as M
from tests import swin_torch as st

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
TOL = {F16: dict(rtol=2e-3, atol=2e-3), BF16: dict(rtol=1.6e-2, atol=1.6e-2)}      # the suite's `close` (tests/test_kernels_gpu.py)
C_MAX = 4.0
C_RMS = 4.0
GRIDS = [(5, 9), (14, 7), (24, 12), (25, 19), (13, 30)]


def _id(v):
    if isinstance(v, torch.dtype):
        return "fp16" if v == F16 else "bf16"
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return None


def close(out, ref, dtype, scale=1.0, msg=""):
    t = TOL[dtype]
    torch.testing.assert_close(out.float().cpu(), ref.float(), rtol=t["rtol"], atol=t["atol"] * scale, msg=lambda m: f"{msg}: {m}")


def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def make_case(dtype, B, H, W, heads, S, seed):
    C = heads * 32
    qkv = randn(B * H * W, 3 * C, seed=seed)
    qkv[:, :2 * C] *= 1.7                                     # q.k / sqrt(32) with a standard deviation of about 3
    table = randn((2 * S - 1) ** 2, heads, seed=seed + 1, scale=1.5)
    pad = randn(2 * C, seed=seed + 2)
    return qkv.to(dtype), table.to(dtype), pad.to(dtype)


def run(dev, qkv, B, H, W, heads, S, shift, table, pad, **kw):
    return ops.attn_swin(qkv.to(dev), B, H, W, heads, table.to(dev), 32 ** -0.5, window=S, shift=shift,
                         pad_kv=None if pad is None else pad.to(dev), **kw)


def bounded(tag, dtype, out, truth, model_rounded):
    e_k = (out.double().cpu() - truth).abs()
    e_m = (model_rounded - truth).abs()
    floor = M.ulp(dtype) * float(truth.abs().max())
    floor_rms = floor / math.sqrt(12.0)
    mk, mm, rk, rm = float(e_k.max()), float(e_m.max()), M.rms(e_k), M.rms(e_m)
    print(f"{tag}: max e_k {mk:.3e} e_m {mm:.3e} floor {floor:.3e}; rms e_k {rk:.3e} e_m {rm:.3e}")
    assert bool(torch.isfinite(out).all()), f"{tag}: non-finite output"
    assert mk <= max(floor, C_MAX * mm), f"{tag}: max error {mk:.3e} > max({floor:.3e}, {C_MAX} * {mm:.3e})"
    assert rk <= max(floor_rms, C_RMS * rm), f"{tag}: rms error {rk:.3e} > max({floor_rms:.3e}, {C_RMS} * {rm:.3e})"


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("S", [7, 12])
@pytest.mark.parametrize("grid", GRIDS, ids=_id)
def test_attn_swin_against_float64(dev, grid, S, shifted, heads, B, dtype):
    H, W = grid
    shift = S // 2 if shifted else 0
    qkv, table, pad = make_case(dtype, B, H, W, heads, S, seed=H * 100 + W + S)
    out = run(dev, qkv, B, H, W, heads, S, shift, table, pad)
    truth = st.attention_from_qkv(qkv.double(), B, H, W, heads, S, shift, table.double(), pad.double())
    model = M.round16(st.attention_from_qkv(qkv.double(), B, H, W, heads, S, shift, table.double(), pad.double(), p_round=dtype), dtype)
    bounded(f"swin {_id(dtype)} {H}x{W} S{S} shift{shift} heads{heads} B{B}", dtype, out, truth, model)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("S", [7, 12])
def test_null_pad_kv_is_zero_keys(dev, S, dtype):
    H, W, heads, B = 13, 9, 2, 1
    qkv, table, _ = make_case(dtype, B, H, W, heads, S, seed=5)
    out = run(dev, qkv, B, H, W, heads, S, S // 2, table, None)
    truth = st.attention_from_qkv(qkv.double(), B, H, W, heads, S, S // 2, table.double(), None)
    model = M.round16(st.attention_from_qkv(qkv.double(), B, H, W, heads, S, S // 2, table.double(), None, p_round=dtype), dtype)
    bounded(f"swin-null-pad {_id(dtype)} S{S}", dtype, out, truth, model)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("S", [7, 12])
@pytest.mark.parametrize("grid", [(5, 9), (25, 19)], ids=_id)
def test_uniform_rows_are_the_window_mean_with_padded_keys(dev, grid, S, dtype):
    """q = 0, table = 0, no shift: every probability is 1 / (S S) — the output is the mean of v over the window INCLUDING the padded
    positions (v = pad_kv) and WITHOUT the keys that only pad 49 to the MFMA tile.  v on the grid of eighths: the sums are exact."""
    H, W = grid
    heads, B, C = 2, 2, 64
    qkv = torch.zeros(B * H * W, 3 * C)
    qkv[:, C:2 * C] = randn(B * H * W, C, seed=3)
    qkv[:, 2 * C:] = torch.round(randn(B * H * W, C, seed=4) * 8.0) / 8.0
    pad = torch.cat([randn(C, seed=6), torch.full((C,), 4.0)])
    table = torch.zeros((2 * S - 1) ** 2, heads)
    out = run(dev, qkv.to(dtype), B, H, W, heads, S, 0, table.to(dtype), pad.to(dtype)).double().cpu().view(B, H, W, C)
    v = F.pad(qkv[:, 2 * C:].to(dtype).double().view(B, H, W, C) - 4.0, (0, 0, 0, (S - W % S) % S, 0, (S - H % S) % S)) + 4.0
    mean = st.partition(v, S).mean(dim=1)                                                     # [B nWy nWx, C]
    nwy, nwx = v.shape[1] // S, v.shape[2] // S
    want = mean.view(B, nwy, 1, nwx, 1, C).expand(B, nwy, S, nwx, S, C).reshape(B, nwy * S, nwx * S, C)[:, :H, :W]
    err = (out - want).abs()
    assert float(err.max()) <= M.ulp(dtype) * float(want.abs().max()), float(err.max())


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("S,grid", [(7, (14, 7)), (12, (24, 12)), (7, (5, 9)), (12, (25, 19))], ids=_id)
def test_shift_mask_keeps_regions_apart(dev, S, grid, dtype):
    """q = 0, table = 0, shift S / 2, v = (the position's region + 1) in every channel, the padded positions included (their v is
    pad_kv, so every region that holds a padded position is given the pad's value): under the -100 mask a query sees its own region
    only (exp(-100) rounds to zero in 16 bits), so its output is its own region's value exactly; without the mask it would be a
    mixture."""
    H, W = grid
    heads, B, C, shift = 1, 1, 32, S // 2
    reg = st.region_of(H, W, S, shift)
    Hp, Wp = -(-H // S) * S, -(-W // S) * S
    val = torch.arange(1, 10, dtype=torch.float32)
    if (Hp, Wp) != (H, W):
        # regions of padded positions: those all take pad v = 16
        full = st.region_of(Hp, Wp, S, shift)
        padded = torch.ones(Hp, Wp, dtype=torch.bool)
        padded[:H, :W] = False
        # a region holding both image and padded positions gets the pad's value on its image positions too
        val[torch.unique(full[padded])] = 16.0
    qkv = torch.zeros(H * W, 3 * C)
    qkv[:, C:2 * C] = randn(H * W, C, seed=8)
    qkv[:, 2 * C:] = val[reg.reshape(-1)][:, None]
    pad = torch.cat([randn(C, seed=9), torch.full((C,), 16.0)])
    # windows, not regions, bound what a query sees: a region's value is constant, so the mean over (window and region) is that value
    out = run(dev, qkv.to(dtype), B, H, W, heads, S, shift, torch.zeros((2 * S - 1) ** 2, heads).to(dtype), pad.to(dtype)).float().cpu()
    want = val[reg.reshape(-1)][:, None].expand(H * W, C)
    assert float((out - want).abs().max()) <= M.ulp(dtype) * 16.0, float((out - want).abs().max())
    assert len(torch.unique(want)) >= 2


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("S", [7, 12])
def test_strided_output_and_canaries(dev, S, dtype):
    """out as a view into a canary-filled buffer with ldo = heads 32 + 8 and rows behind B H W: every canary keeps its bits (columns
    beyond heads 32, rows beyond the grid — the queries of padded positions write nothing), the owned elements equal the dense call's."""
    H, W, heads, B = 13, 17, 3, 2
    C, Mrows = heads * 32, B * H * W
    qkv, table, pad = make_case(dtype, B, H, W, heads, S, seed=11)
    dense = run(dev, qkv, B, H, W, heads, S, S // 2, table, pad)
    buf = torch.full((Mrows + 5, C + 8), -7.25, dtype=dtype, device=dev)
    got = run(dev, qkv, B, H, W, heads, S, S // 2, table, pad, out=buf[:Mrows])
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:Mrows, :C].view(torch.int16), dense.view(torch.int16))
    assert bool((buf[:Mrows, C:] == -7.25).all()) and bool((buf[Mrows:] == -7.25).all())
    # a strided QKV (ld > 3 heads 32) gives the same bits
    wide = torch.zeros((Mrows, 3 * C + 16), dtype=dtype, device=dev)
    wide[:, :3 * C] = qkv.to(dev)
    again = ops.attn_swin(wide[:, :3 * C], B, H, W, heads, table.to(dev), 32 ** -0.5, window=S, shift=S // 2, pad_kv=pad.to(dev))
    assert torch.equal(again.view(torch.int16), dense.view(torch.int16))


def test_batch_and_neighbours_do_not_change_a_window(dev):
    """Sample 1 of a batch of two equals the same sample alone, bit for bit."""
    H, W, heads, S = 25, 19, 3, 12
    qkv, table, pad = make_case(F16, 2, H, W, heads, S, seed=12)
    both = run(dev, qkv, 2, H, W, heads, S, 6, table, pad)
    one = run(dev, qkv[H * W:], 1, H, W, heads, S, 6, table, pad)
    assert torch.equal(both[H * W:], one)


def test_attn_swin_rejects_what_it_cannot_run(dev):
    qkv, table, pad = make_case(F16, 1, 8, 8, 1, 7, seed=13)
    with pytest.raises(L.OmgHipError, match="shift"):
        run(dev, qkv, 1, 8, 8, 1, 7, 2, table, pad)
    with pytest.raises(L.OmgHipError, match="table"):
        run(dev, qkv, 1, 8, 8, 1, 12, 6, table, pad)
    t8 = torch.zeros(15 * 15, 1, dtype=F16)
    with pytest.raises(L.OmgHipError, match="window"):
        run(dev, qkv, 1, 8, 8, 1, 8, 4, t8, pad)


# ------------------------------------------------------------------ patch merging: gather + LayerNorm
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("C", [8, 96, 264, 520])            # 4 C / 8 chunks over 64 lanes: 1, 1, 3 (the 4-chunk form), 5 (the 8-chunk form) per lane
@pytest.mark.parametrize("grid", [(7, 10), (8, 8), (1, 1)], ids=_id)
def test_merge_ln(dev, grid, C, dtype):
    H, W = grid
    B = 2
    x = (randn(B, H, W, C, seed=C + H) * 2.0 + 0.5).to(dtype)
    gamma, beta = (1.0 + 0.2 * randn(4 * C, seed=1)).to(dtype), (0.1 * randn(4 * C, seed=2)).to(dtype)
    y = ops.swin_merge_ln(x.to(dev), gamma.to(dev), beta.to(dev), 1e-5)
    m = st.patch_merge(x.double().view(B, H * W, C), H, W)                                  # zero padding BEFORE the norm
    ref = F.layer_norm(m, (4 * C,), gamma.double(), beta.double(), 1e-5).view(-1, 4 * C)
    assert tuple(y.shape) == (B * ((H + 1) // 2) * ((W + 1) // 2), 4 * C)
    close(y, ref, dtype, scale=2.0, msg=f"merge_ln {H}x{W} C{C}")


def test_merge_ln_rejects_what_it_cannot_run(dev):
    x = torch.zeros(1, 4, 4, 1032, dtype=F16, device=dev)
    g = torch.zeros(4 * 1032, dtype=F16, device=dev)
    with pytest.raises(L.OmgHipError, match="1024"):
        ops.swin_merge_ln(x, g, g, 1e-5)


# ------------------------------------------------------------------ patch rows
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("fp32_in", [True, False])
@pytest.mark.parametrize("size", [(13, 18), (16, 16), (3, 2)], ids=_id)
def test_patch_rows_and_projection(dev, size, fp32_in, dtype):
    H, W = size
    B, E = 2, 32
    x = randn(B, 3, H, W, seed=H + W)
    x = x if fp32_in else x.to(dtype)
    rows = ops.swin_patch_embed(x.to(dev), dtype, 64)
    xp = F.pad(x.to(dtype).double(), (0, (4 - W % 4) % 4, 0, (4 - H % 4) % 4))
    Hg, Wg = xp.shape[2] // 4, xp.shape[3] // 4
    want = xp.view(B, 3, Hg, 4, Wg, 4).permute(0, 2, 4, 1, 3, 5).reshape(B * Hg * Wg, 48)
    assert tuple(rows.shape) == (B * Hg * Wg, 64)
    assert torch.equal(rows[:, :48].double().cpu(), want), "the patch rows are a gather: exact"
    assert bool((rows[:, 48:] == 0).all())
    # with projection.weight.reshape(E, 48) as the GEMM weight the rows are the convolution
    wt, bias = (randn(E, 3, 4, 4, seed=3) * 0.2).to(dtype), (randn(E, seed=4) * 0.1).to(dtype)
    wp = torch.zeros(E, 64, dtype=dtype)
    wp[:, :48] = wt.reshape(E, 48)
    got = ops.gemm(rows, wp.to(dev), bias=bias.to(dev))
    ref = F.conv2d(xp, wt.double(), bias.double(), stride=4).flatten(2).transpose(1, 2).reshape(-1, E)
    close(got, ref, dtype, scale=2.0, msg=f"patch projection {H}x{W}")
