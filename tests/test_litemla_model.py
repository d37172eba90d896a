"""The references of tests/_litemla_model.py, checked without a GPU: the depthwise emulation against float64 conv2d, the rule `held`
against a CPU emulation of the linear-attention kernel with one fault at a time (the evidence that the GPU tests of
tests/test_litemla_conditioning_gpu.py would fail if a kernel were subtly wrong), the identities those tests rely on, and the argument
checks omg_dwconv2d / omg_relu_linear_att do before any launch."""
import pytest
import torch
import torch.nn.functional as F

from omg_amd import _lib
from tests import _litemla_model as M

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]


def _id(v):
    return M.name(v) if isinstance(v, torch.dtype) else None


# ---------------------------------------------------------------------------------------------------------------- depthwise convolution
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("k", [1, 3, 5, 7, 9])
def test_dwconv_emulation_agrees_with_float64_conv2d(dtype, k):
    """fp32 accuracy: a chain of k*k fma and the bias, |error| <= (k*k + 1) 2^-24 (sum |x| |w| + |bias|)."""
    B, C = 2, 24
    for H, W in [(1, 1), (1, 2), (3, 2), (8, 8), (13, 7)]:
        for with_bias in (True, False):
            x, taps, bias = M.dwconv_inputs(B, H, W, C, k, dtype, seed=k + H + W, with_bias=with_bias)
            got = M.dwconv_emulation(x, taps, bias, B, H, W, k).double()
            w = taps.double().t().reshape(C, 1, k, k)
            img = x.double().reshape(B, H, W, C).permute(0, 3, 1, 2)
            ref = F.conv2d(img, w, bias.double() if with_bias else None, padding=k // 2, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
            mag = F.conv2d(img.abs(), w.abs(), bias.double().abs() if with_bias else None, padding=k // 2, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
            assert bool(((got - ref).abs() <= (k * k + 1) * 2.0 ** -24 * mag).all()), (H, W, with_bias, float((got - ref).abs().max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("fault", M.DW_FAULTS)
def test_bitwise_depthwise_comparison_rejects_each_fault(dtype, fault):
    B, H, W, C, k = 2, 5, 4, 8, 3
    x, taps, bias = M.dwconv_inputs(B, H, W, C, k, dtype, seed=5)
    good = M.dwconv_emulation(x, taps, bias, B, H, W, k).to(dtype)
    bad = M.dwconv_emulation(x, taps, bias, B, H, W, k, fault=fault).to(dtype)
    assert not torch.equal(good.view(torch.int16), bad.view(torch.int16))
    if fault == "wrap_batch":       # only the rows next to the seam between the two images differ
        d = (good != bad).reshape(B, H, W * C).any(-1)
        assert d[0, -1] and d[1, 0] and not d[0, :-1].any() and not d[1, 1:].any()


def test_batch_of_three_with_loud_neighbours_shows_a_wrapped_tap():
    """The GPU test's form of the batch check: the middle image of three, the outer ones +-1000, against that image alone."""
    B, H, W, C, k = 3, 3, 2, 8, 5
    x, taps, _ = M.dwconv_inputs(B, H, W, C, k, F16, seed=6, with_bias=False)
    x = x.reshape(B, H * W, C).clone()
    x[0], x[2] = 1000.0, -1000.0
    alone = M.dwconv_emulation(x[1], taps, None, 1, H, W, k).to(F16)
    good = M.dwconv_emulation(x.reshape(-1, C), taps, None, B, H, W, k).to(F16).reshape(B, H * W, C)[1]
    bad = M.dwconv_emulation(x.reshape(-1, C), taps, None, B, H, W, k, fault="wrap_batch").reshape(B, H * W, C)[1].to(F16)
    assert torch.equal(alone, good) and not torch.equal(alone, bad)


# --------------------------------------------------------------------------------------------------------------------- linear attention
def test_ulp16():
    t = torch.tensor([0.0, 1.0, -1.5, 1.9999, 2.0, 2.0 ** -14, 2.0 ** -20, 100.0], dtype=torch.float64)
    assert M.ulp16(t, F16).tolist() == [2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -4]
    assert M.ulp16(t, BF16).tolist() == [2.0 ** -133, 2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -21, 2.0 ** -27, 2.0 ** -1]
    for dtype in DTYPES:          # the spacing really is the distance to the next value of the type
        v = torch.tensor([1.0, 3.0, 100.0, 0.001], dtype=dtype)
        nxt = (v.view(torch.int16) + 1).view(dtype)
        assert torch.equal(nxt.double() - v.double(), M.ulp16(v, dtype))


EMU_SHAPES = [(2, 129, 3, 8), (1, 300, 2, 16), (1, 257, 2, 32), (2, 1, 3, 16)]
EMU_LOG = []


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("kind", M.FAMILIES)
def test_the_unfaulted_emulation_holds_on_every_family(dtype, kind):
    for B, HW, G, dim in EMU_SHAPES:
        for eps in (1e-15, 0.5):
            qkv = M.family(kind, B, HW, G, dim, seed=HW + dim).to(dtype)
            t, r = M.truth(qkv, B, HW, G, dim, eps), M.ref32(qkv, B, HW, G, dim, eps)
            k32 = M.rla_emulation(qkv, B, HW, G, dim, eps)
            rec = M.held(f"emu {kind} {(B, HW, G, dim)} eps {eps}", dtype, k32.to(dtype), t, r, log=EMU_LOG)
            k32_err = float((k32 - t).abs().max())
            rec["k32_over_E32"] = k32_err / rec["E32"] if rec["E32"] > 0 else (0.0 if k32_err == 0 else float("inf"))    # E32 = 0: every row is dead
            # the emulation's fp32 value is visible here: the kernel's summation order is inside the C * E32 the rule grants it
            print(f"{rec['tag']} {rec['dtype']}: k32 / E32 {rec['k32_over_E32']:.2f} excess / E32 {rec['excess_over_E32']:.2f} "
                  f"not round16(truth) {rec['not_round_truth']:.4f}")
            assert rec["k32_over_E32"] <= M.C_RULE, rec


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("kind,fault", [(kind, fault) for kind in ("plain", "sparse_offset") for fault in M.RLA_FAULTS
                                        if (kind, fault) != ("sparse_offset", "relu_v")])      # v = 100 + randn / 4 is positive: no fault there
def test_the_rule_rejects_each_fault(dtype, kind, fault):
    B, HW, G, dim = 2, 129, 3, 16
    eps = 0.5 if fault == "no_eps" else 1e-15
    qkv = M.family(kind, B, HW, G, dim, seed=11).to(dtype)
    t, r = M.truth(qkv, B, HW, G, dim, eps), M.ref32(qkv, B, HW, G, dim, eps)
    M.held(f"good {kind}", dtype, M.rla_emulation(qkv, B, HW, G, dim, eps).to(dtype), t, r)
    with pytest.raises(AssertionError):
        M.held(f"{fault} {kind}", dtype, M.rla_emulation(qkv, B, HW, G, dim, eps, fault=fault).to(dtype), t, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_the_rule_rejects_eps_on_the_wrong_side_and_a_loose_result(dtype):
    B, HW, G, dim, eps = 2, 65, 3, 8, 0.5
    qkv = M.family("plain", B, HW, G, dim, seed=12).to(dtype)
    t, r = M.truth(qkv, B, HW, G, dim, eps), M.ref32(qkv, B, HW, G, dim, eps)
    wrong = M.rla_emulation(qkv, B, HW, G, dim, 0.0) + eps                     # out / den + eps
    with pytest.raises(AssertionError):
        M.held("eps outside", dtype, wrong.to(dtype), t, r)
    one_off = t.to(dtype).clone()                                              # the correctly rounded answer, one element one ulp off
    i = int(torch.argmax(t.abs()))
    one_off.view(torch.int16).view(-1)[i] += 1
    M.held("rounded truth", dtype, t.to(dtype), t, r)
    with pytest.raises(AssertionError):
        M.held("one ulp off", dtype, one_off, t, r)
    nan = t.to(dtype).clone()
    nan.view(-1)[0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        M.held("nan", dtype, nan, t, r)


def _residue_case(B, HW, G, dim, seed=2):
    """k_t = e_(t mod dim), q_t = 2 e_((7 t + 3) mod dim), v integers in -8..8: token t returns the mean of v over the tokens of residue
    class (7 t + 3) mod dim of its own sample and group, exactly."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, HW, G, 3 * dim)
    t = torch.arange(HW)
    x[:, t, :, dim + t % dim] = 1.0
    x[:, t, :, (7 * t + 3) % dim] = 2.0
    x[..., 2 * dim:] = torch.randint(-8, 9, (B, HW, G, dim), generator=g).float()
    cls = x[..., 2 * dim:].permute(0, 2, 1, 3).reshape(B, G, HW // dim, dim, dim).mean(2)       # [B, G, residue, dim]
    want = cls[:, :, (7 * t + 3) % dim].permute(0, 2, 1, 3).reshape(B * HW, G * dim)
    return x.reshape(B * HW, -1), want


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("dim", [8, 16, 32])
def test_residue_classes_are_exact_and_tell_the_faults_apart(dtype, dim):
    B, HW, G = 2, 256, 3
    x, want = _residue_case(B, HW, G, dim)
    assert torch.equal(want, want.to(dtype).float())                           # the means are representable
    qkv = x.to(dtype)
    assert torch.equal(M.rla_emulation(qkv, B, HW, G, dim, 1e-15).to(dtype), want.to(dtype))
    for fault in ("kv_transposed", "skip_last_chunk", "relu_v"):               # k is the same in every group: the groups differ in v (below)
        assert not torch.equal(M.rla_emulation(qkv, B, HW, G, dim, 1e-15, fault=fault).to(dtype), want.to(dtype)), fault
    w = want.reshape(B, HW, G, dim)                                            # another sample or group gives other numbers
    assert not torch.equal(w[0], w[1]) and not torch.equal(w[:, :, 0], w[:, :, 1]) and not torch.equal(w[:, :, 1], w[:, :, 2])


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("dim", [8, 16, 32])
def test_power_of_two_scalings_are_bitwise_in_the_emulation(dtype, dim):
    """q or k times 4 changes no bit (eps = 1e-15 is below half an ulp of every non-zero denominator, and a zero one gives 0 either
    way); v times 4 gives 4 times the output wherever that is a normal number of the type."""
    B, HW, G = 2, 129, 3
    qkv = M.family("plain", B, HW, G, dim, seed=21).to(dtype)
    base = M.rla_emulation(qkv, B, HW, G, dim, 1e-15)
    for part in range(3):
        s = qkv.clone().reshape(B * HW, G, 3, dim)
        s[:, :, part] *= 4
        got = M.rla_emulation(s.reshape(B * HW, -1), B, HW, G, dim, 1e-15)
        assert torch.equal(got, base * 4 if part == 2 else base), part


def test_litemla_entry_points_reject_bad_arguments():
    lib = _lib.lib()
    one, off = 4096, 4096 + 8                                          # stand-in addresses, aligned and 8 bytes off: every call below fails before any launch
    F16_ = _lib.OMG_F16
    def dw(X=one, ldx=16, B=1, H=8, W=8, C=16, k=3, Wt=one, bias=None, Y=one, ldy=16, dtype=F16_):
        return lib.omg_dwconv2d(dtype, X, ldx, B, H, W, C, k, Wt, bias, Y, ldy, None)
    def rla(QKV=one, ld=96, B=1, HW=8, G=2, dim=16, eps=1e-15, ws=one, OUT=one, ldo=32, dtype=F16_):
        return lib.omg_relu_linear_att(dtype, QKV, ld, B, HW, G, dim, eps, ws, OUT, ldo, None)
    assert dw(B=-1) == -1 and dw(H=-1) == -1 and dw(W=-1) == -1           # -1 is OMG_EINVAL: a failed launch would be -3
    assert lib.omg_last_error() == b"omg_dwconv2d: shape"
    assert rla(HW=-1) == -1 and lib.omg_last_error() == b"omg_relu_linear_att: shape"
    assert dw(B=-1, H=-1) == -1                                        # a positive product of two negative counts
    assert dw(X=off) == -1 and dw(Y=off) == -1 and dw(Wt=off) == -1 and dw(bias=off) == -1
    assert dw(k=4) == -1 and dw(k=0) == -1 and dw(k=11) == -1
    assert dw(C=12) == -1 and dw(ldx=8) == -1 and dw(ldy=8) == -1 and dw(X=None) == -1 and dw(dtype=_lib.OMG_F32) == -1
    assert rla(B=-1) == -1 and rla(HW=-1) == -1 and rla(B=-1, HW=-1) == -1
    assert rla(QKV=off) == -1 and rla(OUT=off) == -1 and rla(ws=4096 + 2) == -1
    assert rla(dim=4) == -1 and rla(dim=24) == -1 and rla(dim=64) == -1
    assert rla(ld=88) == -1 and rla(ldo=24) == -1 and rla(G=0) == -1 and rla(ws=None) == -1 and rla(dtype=_lib.OMG_F32) == -1
    # empty work is not an error, and needs no launch
    assert dw(B=0) == 0 and dw(H=0) == 0 and dw(W=0) == 0 and rla(B=0) == 0 and rla(HW=0) == 0
    assert lib.omg_relu_linear_att_ws_floats(2, 3, 16, 129) == 2 * 3 * 2 * 16 * 17
