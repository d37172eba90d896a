"""Every GEMM tile kernel (-m gpu) on every conv mode and operand layout, against tests/_gemm_oracle.py.

The fp16 / bf16 GEMM and implicit-GEMM convolution have seven reachable tile kernels (csrc/gemm.hip ``g_variant``: 1, 13, 14, 15, 24, 25,
28) and a heuristic (0) that picks among them.  Each case here is the smallest at which a tile can go wrong — M = 429 rows (one 256-row
tile + a ragged 173, sample boundaries and image edges inside the tile), N = 328 columns (320 + 8 | 256 + 72 | 2 x 128 + 72) — and runs
under all eight settings and both dtypes, judged four ways:

1. exact: integer operands (see the oracle), ``torch.equal`` with the float64 reference; the message names the first wrong output;
2. canaries: nothing outside the output — the rest of a wider buffer, skipped groups, the image row behind a conv output — changes;
3. bitwise: on random data, SiLU and GEGLU included, every setting returns the bits of variant 1;
4. rounding bound: variant 1 and the heuristic stay inside the derived bound of the oracle on the linear epilogues (by 3, all do).  It
   allows one rounding at the store and fp32 accumulation; it tells one rounding from two everywhere but on the oracle's ``BLIND``
   cases (fp16, K > 576), where it still holds the accumulation.  SiLU and GEGLU keep test_kernels_gpu.py's TOL, their hardware
   approximations are judged in that file.
"""
import contextlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from tests import _gemm_oracle as O
from tests.test_kernels_gpu import TOL

ACT = {"none": L.ACT_NONE, "silu": L.ACT_SILU, "geglu": L.ACT_GEGLU}
CANARY = 1000.0          # representable in both dtypes, larger than any |reference| of the exact cases
FILLER = 3.0             # what surrounds A and W inside their wider buffers: reading it moves an exact sum by a multiple of 3
VID = lambda v: "heuristic" if v == 0 else f"v{v}"
DID = lambda dt: str(dt)[6:]
every_setting = pytest.mark.parametrize("variant", O.SETTINGS, ids=VID)
both_dtypes = pytest.mark.parametrize("dtype", O.DTYPES, ids=DID)

_DEV = {}                # operands on the device, uploaded once per (case, kind, dtype); never written
_BASE = {}               # variant 1's outputs on the random cases: what every other setting must reproduce bit for bit


@contextlib.contextmanager
def forced(variant):
    lib = L.lib()
    lib.omg_debug_set_gemm_variant(variant)
    try:
        yield
    finally:
        lib.omg_debug_set_gemm_variant(0)


def uploaded(key, d, names, dtype, dev):
    if key not in _DEV:
        _DEV[key] = {k: (d[k] if d[k].dtype == torch.int32 else d[k].to(dtype)).to(dev) for k in names if d.get(k) is not None}
    return _DEV[key]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def assert_exact(out, ref, what, conv_shape=None):
    got = out.double().cpu().reshape(ref.shape)
    if torch.equal(got, ref):
        return
    g2, r2 = got.reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    bad = (g2 != r2).nonzero()
    r, c = bad[0].tolist()
    where = f"(row {r}, column {c})"
    if conv_shape is not None:
        _, Ho, Wo, _ = conv_shape
        where += f" = (sample {r // (Ho * Wo)}, y {r % (Ho * Wo) // Wo}, x {r % Wo})"
    pytest.fail(f"{what}: {len(bad)} of {r2.numel()} outputs wrong, rows {int(bad[:, 0].min())}..{int(bad[:, 0].max())}, columns "
                f"{int(bad[:, 1].min())}..{int(bad[:, 1].max())}; first at {where}: got {g2[r, c].item()}, want {r2[r, c].item()}")


def assert_in_bound(out, ref, S, K, K2, dtype, what):
    err = (out.double().cpu().reshape(ref.shape) - ref).abs()
    tol = O.bound(ref, S, K, K2, dtype)
    worst = (err / tol).max().item()
    print(f"{what}: worst error {worst:.3f} x the bound")
    if not bool((err <= tol).all()):          # also true for NaN
        i = (err / tol).flatten().nan_to_num(nan=math.inf).argmax().item()
        pytest.fail(f"{what}: {int((~(err <= tol)).sum())} outputs outside the rounding bound; worst {worst:.2f} x the bound at flat index {i} "
                    f"(column {i % ref.shape[-1]}): error {err.flatten()[i].item():.3e}, bound {tol.flatten()[i].item():.3e}")


def assert_tol(out, ref, dtype, scale=1.0):
    t = TOL[dtype]
    torch.testing.assert_close(out.float().cpu().reshape(ref.shape), ref.float(), rtol=t["rtol"], atol=t["atol"] * scale)


# ------------------------------------------------------------------------------------------------ convolutions
def run_conv(name, kind, dtype, dev, epi):
    d = O.conv_case(name, kind, None if kind == "int" else dtype)
    t = uploaded(("conv", name, kind, dtype), d, ("x1", "x2", "w", "bias", "group_bias", "residual"), dtype, dev)
    e = O.conv_epi_args(d, epi)
    shape = d["out_shape"]
    n = math.prod(shape)
    flat = torch.full((n + shape[2] * shape[3],), CANARY, dtype=dtype, device=dev)      # the output in front of one more image row
    out = flat[:n].view(shape)
    ops.conv2d(t["x1"], t["w"], d["ksize"], x2=t.get("x2"), bias=t["bias"], group_bias=t["group_bias"] if e["group_bias"] is not None else None,
               residual=t["residual"] if e["residual"] is not None else None, out_scale=e["out_scale"], act=ACT[e["act"]], out=out, **d["geo"])
    assert bool((flat[n:] == CANARY).all()), f"conv {name} / {epi}: wrote behind the output"
    return out


@both_dtypes
@every_setting
@pytest.mark.parametrize("name", list(O.CONV_CASES))
def test_conv_is_exact_on_integers(dev, name, variant, dtype):
    for epi in O.LINEAR_EPILOGUES:
        ref, _ = O.conv_expected(name, "int", None, epi)
        with forced(variant):
            out = run_conv(name, "int", dtype, dev, epi)
        assert_exact(out, ref, f"conv {name} / {epi} {DID(dtype)} {VID(variant)}", ref.shape)


@both_dtypes
@every_setting
@pytest.mark.parametrize("name", list(O.CONV_CASES))
def test_conv_on_random_data_is_variant_1_bit_for_bit_and_in_the_rounding_bound(dev, name, variant, dtype):
    for epi in O.CONV_EPILOGUES:
        what = f"conv {name} / {epi} {DID(dtype)} {VID(variant)}"
        key = ("conv", name, dtype, epi)
        if key not in _BASE:
            with forced(1):
                _BASE[key] = run_conv(name, "rnd", dtype, dev, epi)
        with forced(variant):
            out = run_conv(name, "rnd", dtype, dev, epi)
        assert torch.equal(out, _BASE[key]), f"{what}: not the bits of variant 1, max diff {(out.float() - _BASE[key].float()).abs().max().item()}"
        if variant in (0, 1):
            ref, S = O.conv_expected(name, "rnd", dtype, epi)
            if S is not None:
                assert_in_bound(out, ref, S, O.conv_case(name, "rnd", dtype)["K"], 0, dtype, what)
            else:
                assert_tol(out, ref, dtype)


# ------------------------------------------------------------------------------------------------ plain GEMM
def in_wider(x, extra, offset, fill):
    """``x`` [R, C] as the column slice [offset, offset + C) of a new [R, C + extra] buffer filled with ``fill`` -> (buffer, view)."""
    buf = torch.full((x.shape[0], x.shape[1] + extra), fill, dtype=x.dtype, device=x.device)
    view = buf[:, offset:offset + x.shape[1]]
    view.copy_(x)
    return buf, view


def run_gemm(name, kind, dtype, dev, epi):
    """One epilogue of a case -> (out, the down-projection of a LoRA case or None).  Checks the canaries itself."""
    d = O.gemm_case(name, kind, None if kind == "int" else dtype)
    key = ("gemm", name, kind, dtype)
    t = uploaded(key, d, ("a", "w", "bias", "group_bias", "residual", "down", "up", "adapter"), dtype, dev)
    e = O.gemm_epi_args(d, epi)
    M, N, K = d["a"].shape[0], d["w"].shape[-2], d["K"]
    a, w, res = t["a"], t["w"], t["residual"] if e["residual"] is not None else None
    out = wide = before = None
    if d["layouts"]:
        # A = big[:, 32:32+K] of [M, K+64]; W a column slice with ldw = K + 64; out / residual column slices of buffers of different
        # widths (N + 16, N + 40) at an 8-element offset, both filled with the canary.  The residual is only read: a read of its canary
        # moves an output by 1000, and the buffer is compared afterwards all the same.  The output's buffer has one row more than M,
        # so that a write behind the last row's trailing columns lands in it too.
        if "a_view" not in t:
            t["a_view"] = in_wider(t["a"], 64, 32, FILLER)[1]
            t["w_view"] = in_wider(t["w"], 64, 8, FILLER)[1]
            t["res_wide"], t["res_view"] = in_wider(t["residual"], 40, 8, CANARY)
            t["res_before"] = t["res_wide"].clone()
        a, w, res = t["a_view"], t["w_view"], t["res_view"] if res is not None else None
        wide = torch.full((M + 1, N + 16), CANARY, dtype=dtype, device=dev)
        out = wide[:M, 8:8 + N]
        before = wide.clone()
        assert a.stride(0) == K + 64 and w.stride(0) == K + 64 and out.stride(0) == N + 16 and (res is None or res.stride(0) == N + 40)
    elif d["slots"]:
        out = torch.full((M, N), O.OUT_INIT, dtype=dtype, device=dev)
    kw = dict(bias=t["bias"], group_bias=t["group_bias"] if e["group_bias"] is not None else None, residual=res, out_scale=e["out_scale"],
              groups=d["groups"], out=out)
    down = None
    if d["K2"]:
        down = torch.zeros(M, d["K2"], dtype=dtype, device=dev)
        ops.gemm(a, t["down"], out=down, groups=d["groups"], w_group_adapter=t["adapter"])          # N = K2: 8 or 64 columns
        got = ops.gemm(a, w, lora=ops.LoraSpec(down, t["up"], t["adapter"]), **kw)
    elif d["slots"]:
        got = ops.gemm(a, w, w_group_adapter=t["adapter"], **kw)
    else:
        got = ops.gemm(a, w, **kw)
    if wide is not None:
        outside = torch.ones(M + 1, N + 16, dtype=torch.bool, device=dev)
        outside[:M, 8:8 + N] = False
        assert same_bits(wide[outside], before[outside]), f"gemm {name} / {epi}: wrote outside the output's column slice"
        assert same_bits(t["res_wide"], t["res_before"]), f"gemm {name} / {epi}: the residual's buffer changed"
    if d["slots"]:
        rows = M // d["groups"]
        for g, ad in enumerate(d["adapter"].tolist()):
            if ad < 0:
                assert bool((got[g * rows:(g + 1) * rows] == O.OUT_INIT).all()), f"gemm {name} / {epi}: skipped group {g} was written"
    return got, down


@both_dtypes
@every_setting
@pytest.mark.parametrize("name", list(O.GEMM_CASES))
def test_gemm_is_exact_on_integers(dev, name, variant, dtype):
    d = O.gemm_case(name, "int")
    for epi in d["epis"]:
        what = f"gemm {name} / {epi} {DID(dtype)} {VID(variant)}"
        ref, _ = O.gemm_expected(name, "int", None, epi)
        with forced(variant):
            out, down = run_gemm(name, "int", dtype, dev, epi)
        if down is not None:
            assert_exact(down, O.lora_down_ref64(d)[0], what + " (down-projection)")
        assert_exact(out, ref, what)


@both_dtypes
@every_setting
@pytest.mark.parametrize("name", list(O.GEMM_CASES))
def test_gemm_on_random_data_is_variant_1_bit_for_bit_and_in_the_rounding_bound(dev, name, variant, dtype):
    d = O.gemm_case(name, "rnd", dtype)
    for epi in d["epis"]:
        what = f"gemm {name} / {epi} {DID(dtype)} {VID(variant)}"
        key = ("gemm", name, dtype, epi)
        if key not in _BASE:
            with forced(1):
                _BASE[key] = run_gemm(name, "rnd", dtype, dev, epi)
        with forced(variant):
            out, down = run_gemm(name, "rnd", dtype, dev, epi)
        base, base_down = _BASE[key]
        assert torch.equal(out, base), f"{what}: not the bits of variant 1, max diff {(out.float() - base.float()).abs().max().item()}"
        if down is not None:
            assert torch.equal(down, base_down), f"{what}: the down-projection is not variant 1's"
        if variant in (0, 1):
            a2 = None
            if down is not None:
                ref_t, S_t = O.lora_down_ref64(d)
                assert_in_bound(down, ref_t, S_t, d["K"], 0, dtype, what + " (down-projection)")
                a2 = down.cpu()          # the second segment reads THIS 16-bit tensor: the down-projection rounded once to the storage dtype
            ref, S = O.gemm_expected(name, "rnd", dtype, epi, a2=a2)
            assert_in_bound(out, ref, S, d["K"], d["K2"], dtype, what)


@both_dtypes
@every_setting
def test_geglu_on_random_data_is_variant_1_bit_for_bit(dev, variant, dtype):
    """M = 429, N = 128 packed rows -> 64 output columns, K = 192.  Forced 24 / 28 run the 256x256 kernel (a 160-wide wave tile cannot hold
    whole [32 value | 32 gate] blocks).  ``scale=2.0`` on the tolerance as in test_gemm_geglu."""
    d = O.geglu_case(dtype)
    key = ("geglu", dtype)
    if key not in _DEV:
        perm = ops.geglu_row_perm(d["w"].shape[0])
        _DEV[key] = dict(a=d["a"].to(dev), w=d["w"][perm].contiguous().to(dev), bias=d["bias"][perm].contiguous().to(dev))
    t = _DEV[key]
    run = lambda: ops.gemm(t["a"], t["w"], bias=t["bias"], act=L.ACT_GEGLU)
    if key not in _BASE:
        with forced(1):
            _BASE[key] = run()
    with forced(variant):
        out = run()
    assert tuple(out.shape) == (O.GEGLU_CASE["M"], O.GEGLU_CASE["N"] // 2)
    assert torch.equal(out, _BASE[key]), f"geglu {DID(dtype)} {VID(variant)}: not the bits of variant 1, max diff {(out.float() - _BASE[key].float()).abs().max().item()}"
    if variant in (0, 1):
        assert_tol(out, O.gemm_ref64(d["a"], t["w"].cpu(), bias=t["bias"].cpu(), act="geglu"), dtype, scale=2.0)
