"""The CPU model of the fp32 decode path (tests/_conv_f32_model.py) holds its own rule, and the rule and the exact comparison reject each
modelled fault: the proof that tests/test_conv_f32_edges_gpu.py has teeth.  Also the Winograd weight image against a float64 G g G^T
and the refusals the two entry points make before any launch.  No GPU."""
import ctypes as C

import pytest
import torch

from omg_amd import _lib, ops
from tests import _conv_f32_model as M

# (B, H, W, Cin, Cout, upsample): H, W are the INPUT size.  Cout = 68 leaves a partial run behind a 64- and inside a 128-wide block
WINO_SHAPES = [(1, 2, 2, 8, 4, False), (2, 5, 7, 24, 68, True), (1, 6, 10, 128, 60, False), (1, 18, 14, 8, 12, False)]
DIRECT_SHAPES = [(1, 1, 1, 32, 4, 1, False), (2, 5, 7, 32, 68, 3, True), (1, 6, 10, 128, 132, 3, False), (3, 3, 5, 64, 8, 1, False)]
FAULT_SHAPE = (2, 5, 7, 32, 68, True)


def _offset_1000(x, kind):
    return x + 900.0 if kind == "offset1000" else x


@pytest.mark.parametrize("kind", M.FAMILIES + ("offset1000",))
@pytest.mark.parametrize("shape", WINO_SHAPES, ids=str)
def test_winograd_emulation_holds_the_rule(shape, kind):
    B, H, W, Cin, Cout, ups = shape
    x, w, b, r = M.make_case("offset" if kind == "offset1000" else kind, B, H, W, Cin, Cout, 3, ups, True, True, seed=1)
    x = _offset_1000(x, kind)
    ref, _ = M.reference(x, w, b, r, 3, ups)
    got = M.wino_emulation(x, w, b, r, ups)
    h = M.held(got.double() - ref, M.wino_magnitude(x, w, b, r, ups), Cin, M.C_WINO)
    print(f"winograd emulation {shape} {kind}: worst {h.worst:.3f} x the bound, rms {h.rms:.3f}")
    assert h.ok, h
    if kind == "int":
        assert M.first_mismatch(got, ref) is None


@pytest.mark.parametrize("kind", M.FAMILIES + ("offset1000",))
@pytest.mark.parametrize("shape", DIRECT_SHAPES, ids=str)
def test_direct_emulation_holds_the_rule(shape, kind):
    B, H, W, Cin, Cout, k, ups = shape
    x, w, b, r = M.make_case("offset" if kind == "offset1000" else kind, B, H, W, Cin, Cout, k, ups, True, True, seed=2)
    x = _offset_1000(x, kind)
    ref, S = M.reference(x, w, b, r, k, ups)
    got = M.direct_emulation(x, w, b, r, k, ups)
    h = M.held(got.double() - ref, S, k * k * Cin, M.C_DIRECT)
    print(f"direct emulation {shape} {kind}: worst {h.worst:.3f} x the bound, rms {h.rms:.3f}")
    assert h.ok, h
    if kind == "int":
        assert M.first_mismatch(got, ref) is None


def test_the_magnitudes_are_what_they_say():
    """S >= |reference| and S_w >= S_w's own sum without the absolute values (= the reference): both are sums of the moduli of the terms
    of an exact evaluation.  Without bias and residual an all-positive input with all-positive weights has S = reference."""
    x, w, b, r = M.make_case("randn", 2, 4, 6, 16, 12, 3, False, True, True, seed=3)
    ref, S = M.reference(x, w, b, r, 3, False)
    Sw = M.wino_magnitude(x, w, b, r, False)
    assert bool((S >= ref.abs()).all()) and bool((Sw * (1 + 1e-12) >= ref.abs()).all())
    ref, S = M.reference(x.abs(), w.abs(), None, None, 3, False)
    assert torch.allclose(ref, S, rtol=1e-14, atol=0)
    got = M.wino_emulation(x, w, None, None, False)                 # and the emulation without bias / residual is the same convolution
    assert M.held(got.double() - M.reference(x, w, None, None, 3, False)[0], M.wino_magnitude(x, w, None, None, False), 16, M.C_WINO).ok


@pytest.mark.parametrize("fault", M.FAULTS)
def test_winograd_faults_are_rejected(fault):
    B, H, W, Cin, Cout, ups = FAULT_SHAPE
    x, w, b, r = M.make_case("int", B, H, W, Cin, Cout, 3, ups, True, True, seed=4)
    ref, _ = M.reference(x, w, b, r, 3, ups)
    if fault != "mantissa10":                                       # integers up to 3 survive a 10-bit mantissa
        msg = M.first_mismatch(M.wino_emulation(x, w, b, r, ups, fault=fault), ref)
        assert msg is not None and "first at (sample" in msg, fault
    for cin in (Cin, 128):
        x, w, b, r = M.make_case("randn", B, H, W, cin, Cout, 3, ups, True, True, seed=5)
        ref, _ = M.reference(x, w, b, r, 3, ups)
        h = M.held(M.wino_emulation(x, w, b, r, ups, fault=fault).double() - ref, M.wino_magnitude(x, w, b, r, ups), cin, M.C_WINO)
        print(f"winograd fault {fault}, Cin {cin}: worst {h.worst:.3g} x the bound, rms {h.rms:.3g}")
        assert not h.ok, (fault, cin, h)


@pytest.mark.parametrize("fault", M.DIRECT_FAULTS)
def test_direct_faults_are_rejected(fault):
    B, H, W, Cin, Cout, ups = FAULT_SHAPE
    x, w, b, r = M.make_case("int", B, H, W, Cin, Cout, 3, ups, True, True, seed=6)
    ref, _ = M.reference(x, w, b, r, 3, ups)
    if fault != "mantissa10":
        msg = M.first_mismatch(M.direct_emulation(x, w, b, r, 3, ups, fault=fault), ref)
        assert msg is not None and "first at (sample" in msg, fault
    for cin in (Cin, 128):
        x, w, b, r = M.make_case("randn", B, H, W, cin, Cout, 3, ups, True, True, seed=7)
        ref, S = M.reference(x, w, b, r, 3, ups)
        h = M.held(M.direct_emulation(x, w, b, r, 3, ups, fault=fault).double() - ref, S, 9 * cin, M.C_DIRECT)
        print(f"direct fault {fault}, Cin {cin}: worst {h.worst:.3g} x the bound, rms {h.rms:.3g}")
        assert not h.ok, (fault, cin, h)


def test_the_zero_sum_family_tells_the_order_of_the_input_transform():
    """With B^T d B rows first throughout, the rounding of d1 + d2 (about 200 on the offset input) comes out of the column differences as
    an error relative to |V| of order 1: the positions whose U does not cancel carry it into the output.  Invisible where |U11| |V11|
    dominates S_w (any filter whose taps do not sum to zero), inside the rule from Cin = 32 on; at Cin = 8 the rule rejects it."""
    B, H, W, Cin, Cout, ups = 1, 18, 14, 8, 12, False
    x, w, b, r = M.make_case("zero_sum", B, H, W, Cin, Cout, 3, ups, True, True, seed=9)
    ref, _ = M.reference(x, w, b, r, 3, ups)
    Sw = M.wino_magnitude(x, w, b, r, ups)
    bad = M.held(M.wino_emulation(x, w, b, r, ups, fault=M.ROWS_FIRST).double() - ref, Sw, Cin, M.C_WINO)
    good = M.held(M.wino_emulation(x, w, b, r, ups).double() - ref, Sw, Cin, M.C_WINO)
    print(f"zero_sum, Cin 8: rows first {bad.worst:.3f} / {bad.rms:.3f}, differences first {good.worst:.3f} / {good.rms:.3f}")
    assert good.ok and not bad.ok and bad.rms > 4 * good.rms
    x, w, b, r = M.make_case("int", B, H, W, Cin, Cout, 3, ups, True, True, seed=9)
    assert M.first_mismatch(M.wino_emulation(x, w, b, r, ups, fault=M.ROWS_FIRST), M.reference(x, w, b, r, 3, ups)[0]) is None


def test_held_counts_every_element():
    S = torch.ones(1, 2, 2, 4, dtype=torch.float64)
    err = torch.zeros_like(S)
    assert M.held(err, S, 8, 4).ok
    err[0, 1, 1, 3] = 13 * M.U24                                    # one element over (8 + 4) u S
    assert not M.held(err, S, 8, 4).ok
    err[0, 1, 1, 3] = float("nan")
    assert not M.held(err, S, 8, 4).ok
    err = torch.full_like(S, 3 * M.U24)                             # every element inside (8 + 4) u S, the rms over sqrt(8) u
    h = M.held(err, S, 8, 4)
    assert h.worst < 1 and h.rms > 1 and not h.ok
    S[0, 0, 0, 0], err = 0.0, torch.zeros_like(S)
    assert M.held(err, S, 8, 4).ok
    err[0, 0, 0, 0] = 1e-30                                         # nothing went into this output: any error is one
    assert not M.held(err, S, 8, 4).ok


@pytest.mark.parametrize("cout", [4, 60, 64, 68])
@pytest.mark.parametrize("cin", [8, 24])
def test_pack_conv_weight_wino_is_g_g_gt_in_the_documented_layout(cout, cin):
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
    idx = M.wino_layout_index(cout, cin)
    nb = (cout + 63) // 64
    for kind in ("int", "randn"):
        _, w, _, _ = M.make_case(kind, 1, 2, 2, cin, cout, 3, False, False, False, seed=8)
        img = ops.pack_conv_weight_wino(w)
        assert img.dtype == torch.float32 and img.numel() == nb * (cin // 8) * 16 * 2 * 64 * 4 == idx.numel()
        assert torch.equal(idx.flatten().sort().values, torch.arange(img.numel()))        # the formula is a bijection onto the image
        got = img[idx].double()                                                              # [64 nb, cin, 16]
        want = (G @ w.double() @ G.t()).reshape(cout, cin, 16)
        assert torch.equal(got[cout:], torch.zeros(nb * 64 - cout, cin, 16, dtype=torch.float64))       # the rows the kernel's last block pads
        if kind == "int":
            assert torch.equal(got[:cout], want)
        else:
            assert bool(((got[:cout] - want).abs() <= M.U24 * want.abs()).all())          # one rounding of the float64 value


def test_conv2d_f32_entry_points_refuse_before_any_launch():
    lib = _lib.lib()
    one = 4096                                                          # a stand-in address: every call below fails before any launch

    def direct(**kw):
        a = _lib.Conv2dF32Args()
        f = dict(B=1, Hin=4, Win=4, Cin=32, Hout=4, Wout=4, Cout=8, ksize=3, upsample=0, X=one, W=one, bias=None, residual=None, Y=one)
        f.update(kw)
        for k, v in f.items():
            setattr(a, k, v)
        return lib.omg_conv2d_f32(C.byref(a), None)

    def wino(**kw):
        a = _lib.Conv2dF32WinoArgs()
        f = dict(B=1, Hin=4, Win=4, Cin=8, Hout=4, Wout=4, Cout=8, upsample=0, X=one, U=one, bias=None, residual=None, Y=one)
        f.update(kw)
        for k, v in f.items():
            setattr(a, k, v)
        return lib.omg_conv2d_f32_wino(C.byref(a), None)

    EINVAL = -1                                                         # a failed launch would be -3
    assert lib.omg_conv2d_f32(None, None) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32: null args"
    assert direct(ksize=2) == EINVAL and direct(ksize=5) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32: ksize must be 1 or 3"
    for kw in (dict(Cin=8), dict(Cin=24), dict(Cin=48), dict(Cin=0), dict(Cout=6), dict(Cout=130)):
        assert direct(**kw) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32: Cin % 32, Cout % 4", kw
    for kw in (dict(X=None), dict(W=None), dict(Y=None)):
        assert direct(**kw) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32: null operand", kw
    for kw in (dict(Hout=5), dict(Wout=3), dict(Hout=8, Wout=8), dict(upsample=1), dict(upsample=1, Hout=8)):
        assert direct(**kw) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32: stride 1, 'same' padding only", kw
    assert direct(B=0) == 0 and direct(Hin=0, Hout=0) == 0              # empty work is not an error, and needs no launch

    assert lib.omg_conv2d_f32_wino(None, None) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32_wino: null args"
    for kw in (dict(Cin=4), dict(Cin=12), dict(Cin=0), dict(Cout=6), dict(Cout=0), dict(Cout=66)):
        assert wino(**kw) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32_wino: Cin % 8, Cout % 4", kw
    for kw in (dict(X=None), dict(U=None), dict(Y=None)):
        assert wino(**kw) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32_wino: null operand", kw
    for kw in (dict(Hout=6), dict(Wout=2), dict(upsample=1), dict(upsample=1, Hout=8)):
        assert wino(**kw) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32_wino: 3x3, stride 1, 'same' padding only", kw
    for kw in (dict(Hin=3, Hout=3), dict(Win=5, Wout=5), dict(Hin=1, Win=1, Hout=1, Wout=1)):
        assert wino(**kw) == EINVAL and lib.omg_last_error() == b"omg_conv2d_f32_wino: even output sizes only (2x2 tiles)", kw
    assert wino(B=0) == 0 and wino(Hin=0, Hout=0) == 0
    assert lib.omg_conv2d_f32_wino_weight_floats(68, 24) == 2 * 3 * 16 * 2 * 64 * 4


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("cols", [1, 2, 255, 256, 257, 1000, 16384])
def test_softmax_emulation_holds_its_bound(dtype, cols):
    g = torch.Generator().manual_seed(cols)
    x = (torch.randn(5, cols, generator=g) * 3).to(dtype)
    for scale in (1.0, 0.37):
        p = M.softmax_truth(x, scale)
        err = (M.softmax_emulation(x, scale).double() - p).abs()
        tol = M.softmax_bound(p, cols, dtype)
        print(f"softmax emulation {cols} {dtype} x{scale}: worst {(err / tol).max().item():.3f} x the bound")
        assert bool((err <= tol).all())
    eq = torch.full((2, cols), 2.0, dtype=dtype)                    # powers of two: the exponent is exactly 0, the sum exactly cols
    assert torch.equal(M.softmax_emulation(eq, 0.5), torch.full((2, cols), 1.0 / cols, dtype=torch.float64).to(dtype))
