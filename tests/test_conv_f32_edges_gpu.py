"""conv_f32_kernel (csrc/gemm_f32.hip) and conv_f32_wino_kernel (csrc/conv_f32_wino.hip) at their tile edges: every case is tiny and is
there for a branch of one of the kernels (comments in the case lists).  Reference everywhere: the float64 convolution of
tests/_conv_f32_model.py — never the other kernel, never the emulation.  Checks: the integer family exactly; randn, offset and zero-sum
inputs under `held` (derived in the model's docstring; tests/test_conv_f32_model.py shows that it rejects each modelled fault); a marker
behind the output; batch independence and the reach of one NaN bit for bit; what algo="auto" launches."""
import pytest
import torch

from omg_amd import ops
from tests import _conv_f32_model as M

pytestmark = pytest.mark.gpu

T, F_ = True, False
# (B, Hin, Win, Cin, Cout, upsample, bias, residual) — Hin, Win are the INPUT size; the output is twice that with upsample.
# Winograd: nk = Cin / 8 K stages (1, 2, 3 run the prologue alone / one / two turns of the double buffer: Cin 8, 16, 24 exist for this kernel
# only), 64-channel blocks (Cout 4, 60: one partial block, `c >= Cout` skips 15 / 1 runs of 4 and the packed image has zero rows; 68, 132:
# a full block and a partial one), 16 x 16 patches of 2 x 2 tiles (`oy >= Hout` / `ox >= Wout` return).
WINO_CASES = [
    (1, 2, 2, 8, 4, F_, T, T),          # less than one patch: 63 of 64 tiles return; nk = 1: no second stage at all; one run of 4 channels
    (3, 2, 34, 8, 64, F_, F_, F_),      # one tile row, three patches across, the last 2 pixels wide; no bias, no residual
    (1, 1, 1, 8, 132, T, T, F_),        # upsample 1x1 -> 2x2: every tap of the 4x4 patch is pixel 0 or padding
    (1, 16, 16, 16, 4, F_, T, T),       # exactly one full patch; nk = 2: `if (nk > 1)` taken, `kt + 2 < nk` never
    (1, 18, 14, 16, 64, F_, F_, T),     # a second patch row of one tile row, 14 = one tile short of a patch
    (3, 5, 9, 16, 68, T, T, T),         # upsample from odd sizes: the last row reads iy >> 1 = 4 and row 10 is padding; 10 x 18 output
    (1, 30, 50, 24, 60, F_, T, F_),     # nk = 3: both `kt + 1 < nk` and `kt + 2 < nk` change inside the loop; 2 x 4 patches, partial both ways
    (1, 9, 8, 24, 64, T, F_, T),        # upsample to 18 x 16
    (3, 16, 16, 24, 132, F_, T, T),     # three channel blocks share each patch (channel blocks fastest in the block index)
    (1, 2, 2, 32, 64, F_, T, T),
    (1, 18, 14, 32, 60, F_, T, T),
    (1, 5, 9, 32, 132, T, F_, F_),
    (3, 2, 34, 40, 4, F_, T, T),        # Cin = 40: nk = 5 is odd, the last stage computes from buffer 0
    (1, 16, 16, 40, 64, F_, T, T),
    (1, 30, 50, 40, 68, F_, T, T),      # 16 workgroups: two per XCD
    (1, 2, 34, 128, 60, F_, T, T),      # the decode's own depth of K
    (1, 9, 8, 128, 64, T, T, T),
    (1, 18, 14, 128, 68, F_, F_, T),
    (1, 1, 17, 8, 60, T, T, T),         # each remaining output size once with upsample: 2 x 34 ...
    (1, 8, 8, 16, 64, T, T, T),         # ... 16 x 16 ...
    (1, 9, 7, 24, 4, T, T, T),          # ... 18 x 14 ...
    (1, 15, 25, 8, 68, T, T, T),        # ... 30 x 50, from odd sizes
    (5, 2, 2, 8, 64, F_, T, T),         # 5 and ...
    (7, 1, 1, 16, 4, T, T, T),          # ... 7 workgroups: the residues mod 8 of the XCD remap that B in {1, 3} cannot make
    (3, 30, 50, 8, 4, F_, F_, T),       # 24 workgroups = 0 mod 8: the remap is a plain transpose
    (1, 2, 34, 16, 132, F_, T, F_),     # 9 workgroups = 1 mod 8
    (1, 5, 9, 40, 60, T, T, T),         # 2 workgroups
    (1, 18, 14, 8, 132, F_, T, T),      # 6 workgroups
]
WINO_CIN, WINO_COUT = {8, 16, 24, 32, 40, 128}, {4, 60, 64, 68, 132}
WINO_OUT = {(2, 2), (2, 34), (16, 16), (18, 14), (30, 50)}
WINO_UPS_FROM = {(1, 1), (5, 9), (9, 8)}

# (B, Hin, Win, Cin, Cout, ksize, upsample, bias, residual).  Direct kernel: 128 x 128 tiles of M = B Hout Wout rows x Cout, K stages of 32
# (`cpt` = Cin / 32 stages per tap), rows beyond M clamped to M - 1 on the way in and skipped on the way out.
DIRECT_CASES = [
    (1, 1, 1, 32, 4, 1, F_, T, T),          # M = 1, one stage in all (nk = 1: the loop's only turn issues the stage past the end), one run of 4 channels
    (1, 1, 1, 64, 124, 3, F_, F_, F_),      # a 1x1 image under a 3x3 filter: eight of nine taps are padding; Cout one run under a tile; no bias, no residual
    (40, 2, 2, 32, 132, 3, F_, T, F_),      # M = 160: the first tile spans 32 images (cb = 0..31), the second tile 32 rows; Cout one run over a tile
    (40, 2, 2, 96, 128, 1, F_, F_, T),      # the same rows through the 1x1 path, cpt = 3
    (3, 3, 5, 64, 132, 3, F_, T, T),        # odd sizes, M = 45
    (3, 3, 5, 32, 124, 3, T, T, T),         # upsample from odd sizes to 6 x 10, M = 180: a tile boundary inside image 2
    (1, 11, 12, 96, 4, 3, F_, T, T),        # M = 132 = one tile + 4 rows
    (1, 11, 12, 32, 128, 1, F_, F_, F_),
    (2, 16, 16, 64, 128, 3, F_, T, T),      # full tiles only: 4 x 1
    (2, 16, 16, 96, 132, 1, F_, T, F_),     # 4 x 2 tiles = 0 mod 8 workgroups
    (1, 1, 1, 96, 132, 3, T, F_, T),        # upsample 1x1 -> 2x2
    (40, 1, 1, 64, 4, 3, T, T, T),          # the same with a tile across 32 images
]
DIRECT_BHW = {(1, 1, 1), (40, 2, 2), (3, 3, 5), (1, 11, 12), (2, 16, 16)}
RULE_FAMILIES = ("randn", "offset", "zero_sum")
MARKER = -12345.625


def _id(c):
    return "x".join(str(int(v)) for v in c)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _cout_class(cout):
    return "partial" if cout < 64 else "full" if cout % 64 == 0 else "full+partial"


def _wino_wgs(c):
    B, H, W, _, Cout, ups = c[:6]
    Ho, Wo = M.out_size(H, W, ups)
    return B * ((Ho + 15) // 16) * ((Wo + 15) // 16) * ((Cout + 63) // 64)


def test_the_case_lists_cover_what_they_are_there_for():
    assert {c[3] for c in WINO_CASES} == WINO_CIN and {c[4] for c in WINO_CASES} == WINO_COUT
    assert {(c[3], _cout_class(c[4])) for c in WINO_CASES} == {(ci, k) for ci in WINO_CIN for k in ("partial", "full", "full+partial")}
    assert {M.out_size(c[1], c[2], c[5]) for c in WINO_CASES if not c[5]} == WINO_OUT
    assert {M.out_size(c[1], c[2], c[5]) for c in WINO_CASES if c[5]} >= WINO_OUT            # every size once with upsample
    assert {(c[1], c[2]) for c in WINO_CASES if c[5]} >= WINO_UPS_FROM
    assert {c[0] for c in WINO_CASES} >= {1, 3}
    assert {(c[6], c[7]) for c in WINO_CASES} == {(T, T), (T, F_), (F_, T), (F_, F_)}
    assert {_wino_wgs(c) % 8 for c in WINO_CASES} == set(range(8))                            # every residue of the XCD remap
    assert all(M.out_size(c[1], c[2], c[5])[0] % 2 == 0 and M.out_size(c[1], c[2], c[5])[1] % 2 == 0 for c in WINO_CASES)
    assert {c[3] for c in DIRECT_CASES} == {32, 64, 96} and {c[4] for c in DIRECT_CASES} == {4, 124, 128, 132}
    assert {c[5] for c in DIRECT_CASES} == {1, 3} and {c[:3] for c in DIRECT_CASES if not c[6]} == DIRECT_BHW
    assert {(c[1], c[2]) for c in DIRECT_CASES if c[6]} == {(3, 5), (1, 1)}
    assert {(c[7], c[8]) for c in DIRECT_CASES} == {(T, T), (T, F_), (F_, T), (F_, F_)}


def _run(dev, algo, x, w, b, r, ksize, ups, wu=None):
    """The kernel into the front of a larger buffer full of a marker: -> (output on the CPU, what lies behind it).  The output's last
    rows are where a partial patch / a partial channel block / the rows beyond M would spill."""
    B, H, W, _ = x.shape
    Ho, Wo = M.out_size(H, W, ups)
    n = B * Ho * Wo * w.shape[0]
    buf = torch.full((n + 8192,), MARKER, dtype=torch.float32, device=dev)
    wd = w.to(dev)
    if algo != "direct" and wu is None and ksize == 3:
        wu = ops.pack_conv_weight_wino(wd)
    y = ops.conv2d_f32(x.to(dev), ops.pack_conv_weight(wd), ksize, upsample=ups, bias=None if b is None else b.to(dev),
                       residual=None if r is None else r.to(dev), algo=algo, wu=wu, out=buf[:n].view(B, Ho, Wo, -1))
    assert y.data_ptr() == buf.data_ptr()
    return y.cpu(), buf[n:].cpu()


def _assert_untouched(tail, what):
    assert bool((tail == MARKER).all()), f"{what}: {int((tail != MARKER).sum())} floats behind the output were written"


def _check_case(dev, algo, case, ksize):
    B, H, W, Cin, Cout, ups, bias, res = case
    what = f"{algo} {_id(case)} k{ksize}"
    wino = algo == "winograd"
    x, w, b, r = M.make_case("int", B, H, W, Cin, Cout, ksize, ups, bias, res, seed=11)
    y, tail = _run(dev, algo, x, w, b, r, ksize, ups)
    assert ops.LAST_CONV2D_F32_ALGO == algo
    _assert_untouched(tail, what)
    msg = M.first_mismatch(y, M.reference(x, w, b, r, ksize, ups)[0])
    assert msg is None, f"{what}, int: {msg}"
    for kind in RULE_FAMILIES:
        x, w, b, r = M.make_case(kind, B, H, W, Cin, Cout, ksize, ups, bias, res, seed=12)
        y, tail = _run(dev, algo, x, w, b, r, ksize, ups)
        _assert_untouched(tail, what)
        ref, S = M.reference(x, w, b, r, ksize, ups)
        if wino:
            h = M.held(y.double() - ref, M.wino_magnitude(x, w, b, r, ups), Cin, M.C_WINO)
        else:
            h = M.held(y.double() - ref, S, ksize * ksize * Cin, M.C_DIRECT)
        print(f"RATIO {algo} {kind} {_id(case)} k{ksize}: worst err / bound {h.worst:.4f}, rms ratio {h.rms:.4f}")
        assert h.ok, (what, kind, h)


@pytest.mark.parametrize("case", WINO_CASES, ids=_id)
def test_winograd_exact_on_integers_and_inside_the_rounding_rule(dev, case):
    _check_case(dev, "winograd", case, 3)


@pytest.mark.parametrize("case", DIRECT_CASES, ids=_id)
def test_direct_exact_on_integers_and_inside_the_rounding_rule(dev, case):
    B, H, W, Cin, Cout, k, ups, bias, res = case
    _check_case(dev, "direct", (B, H, W, Cin, Cout, ups, bias, res), k)


def _bits(t):
    return t.contiguous().view(torch.int32)


# (algo, B = 3 or more, Hin, Win, Cin, Cout, ksize, upsample): the direct cases whose tiles span images are the 2x2 / 1x1 / 3x5 ones
BATCH_CASES = [("winograd", 3, 2, 34, 8, 60, 3, F_), ("winograd", 3, 5, 9, 24, 68, 3, T), ("winograd", 3, 18, 14, 16, 132, 3, F_),
               ("direct", 40, 2, 2, 32, 132, 3, F_), ("direct", 40, 1, 1, 64, 4, 3, T), ("direct", 3, 3, 5, 32, 124, 3, T),
               ("direct", 3, 3, 5, 64, 132, 1, F_), ("direct", 3, 16, 16, 32, 128, 3, F_)]


@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: c[0] + "-" + _id(c[1:]))
def test_an_image_does_not_depend_on_its_batch(dev, case):
    """y[b] of the batched call equals the call on image b alone, bit for bit: each output's products and their order are the same
    wherever its tile lies."""
    algo, B, H, W, Cin, Cout, k, ups = case
    x, w, b, r = M.make_case("randn", B, H, W, Cin, Cout, k, ups, True, True, seed=13)
    y, _ = _run(dev, algo, x, w, b, r, k, ups)
    for i in sorted({0, 1, B // 2, B - 1}):
        yi, _ = _run(dev, algo, x[i:i + 1].contiguous(), w, b, r[i:i + 1].contiguous(), k, ups)
        assert torch.equal(_bits(y[i]), _bits(yi[0])), (case, i)


# (algo, B, Hin, Win, Cin, Cout, upsample, image, [(y, x) of the NaN in the INPUT]): a corner, the patch seam (x = 15 / 16), the last partial
# patch; for the direct kernel the seam is the tile boundary (row 127 / 128 of M = image 0, (7, 15) / (8, 0) at 16 x 16)
NAN_CASES = [("winograd", 3, 30, 50, 8, 68, F_, 1, [(0, 0), (7, 15), (7, 16), (15, 15), (16, 16), (29, 49), (20, 48), (29, 0)]),
             ("winograd", 3, 9, 8, 16, 60, T, 2, [(0, 0), (8, 7), (7, 7), (4, 3)]),
             ("winograd", 1, 2, 2, 8, 4, F_, 0, [(0, 0), (1, 1)]),
             ("direct", 2, 16, 16, 32, 132, F_, 0, [(0, 0), (7, 15), (8, 0), (15, 15)]),
             ("direct", 40, 2, 2, 32, 4, F_, 31, [(0, 0), (1, 1)]),
             ("direct", 3, 3, 5, 32, 124, T, 2, [(0, 0), (2, 4), (0, 2)])]


@pytest.mark.parametrize("case", NAN_CASES, ids=lambda c: c[0] + "-" + _id(c[1:8]))
def test_one_nan_reaches_its_neighbourhood_and_nothing_else(dev, case):
    """One NaN in one channel of one input pixel: outputs farther than 1 pixel (direct) or 2 pixels (Winograd: the 4x4 patch of a
    2x2 tile) from the pixel's footprint, and every other image, are bit-identical to the clean run; the pixel's own output is NaN."""
    algo, B, H, W, Cin, Cout, ups, img, spots = case
    x, w, b, r = M.make_case("randn", B, H, W, Cin, Cout, 3, ups, True, True, seed=14)
    clean, _ = _run(dev, algo, x, w, b, r, 3, ups)
    assert bool(torch.isfinite(clean).all())
    Ho, Wo = M.out_size(H, W, ups)
    reach, f = (2 if algo == "winograd" else 1), (2 if ups else 1)
    oy, ox = torch.arange(Ho).view(Ho, 1), torch.arange(Wo).view(1, Wo)
    for (py, px) in spots:
        xn = x.clone()
        xn[img, py, px, 3] = float("nan")
        y, tail = _run(dev, algo, xn, w, b, r, 3, ups)
        _assert_untouched(tail, case)
        dist = torch.maximum(torch.maximum(py * f - oy, oy - (py * f + f - 1)), torch.maximum(px * f - ox, ox - (px * f + f - 1)))
        far = (dist > reach).view(1, Ho, Wo, 1).expand(B, Ho, Wo, Cout).clone()
        far[torch.arange(B) != img] = True
        same = _bits(y) == _bits(clean)
        assert bool(same[far].all()), (case[:8], (py, px), f"{int((~same & far).sum())} outputs outside the NaN's reach changed")
        assert bool(torch.isnan(y[img, py * f, px * f]).all()), (case[:8], (py, px), "the NaN did not reach its own pixel")


def test_auto_is_winograd_where_it_applies_and_direct_exactly_elsewhere(dev):
    """algo="auto" with the fill threshold at 0: the same bits as algo="winograd" wherever wino_ok holds, the direct kernel exactly where it
    does not (1x1 filter, an odd output size, no weight image)."""
    ops.set_conv2d_f32_auto(True, 0)
    try:
        for case in [WINO_CASES[0], WINO_CASES[5], WINO_CASES[6], (3, 16, 16, 32, 132, F_, T, T)]:
            B, H, W, Cin, Cout, ups, bias, res = case
            x, w, b, r = M.make_case("randn", B, H, W, Cin, Cout, 3, ups, bias, res, seed=15)
            ya, _ = _run(dev, "auto", x, w, b, r, 3, ups)
            assert ops.LAST_CONV2D_F32_ALGO == "winograd", case
            yw, _ = _run(dev, "winograd", x, w, b, r, 3, ups)
            assert torch.equal(_bits(ya), _bits(yw)), case
        # (B, Hin, Win, Cin, Cout, ksize, upsample, pass the weight image)
        for (B, H, W, Cin, Cout, k, ups, with_wu) in [(1, 4, 4, 32, 8, 1, F_, F_), (1, 3, 5, 32, 8, 3, F_, T), (1, 4, 5, 32, 8, 3, F_, T),
                                                       (1, 4, 4, 32, 8, 3, F_, F_), (1, 3, 5, 32, 8, 1, T, F_)]:
            x, w, b, r = M.make_case("randn", B, H, W, Cin, Cout, k, ups, True, True, seed=16)
            wu = ops.pack_conv_weight_wino(w.to(dev)) if with_wu else None
            ya, _ = _run(dev, "auto", x, w, b, r, k, ups, wu=wu) if with_wu else _run_no_wu(dev, x, w, b, r, k, ups)
            assert ops.LAST_CONV2D_F32_ALGO == "direct", (B, H, W, Cin, Cout, k, ups, with_wu)
            yd, _ = _run(dev, "direct", x, w, b, r, k, ups)
            assert torch.equal(_bits(ya), _bits(yd))
            with pytest.raises(Exception):
                _run(dev, "winograd", x, w, b, r, k, ups, wu=wu) if with_wu else _run_no_wu(dev, x, w, b, r, k, ups, algo="winograd")
        ops.set_conv2d_f32_auto(False, 0)                               # switched off: direct even where Winograd applies
        x, w, b, r = M.make_case("randn", 1, 16, 16, 32, 64, 3, F_, True, True, seed=17)
        _run(dev, "auto", x, w, b, r, 3, F_)
        assert ops.LAST_CONV2D_F32_ALGO == "direct"
    finally:
        ops.set_conv2d_f32_auto()


def _run_no_wu(dev, x, w, b, r, ksize, ups, algo="auto"):
    y = ops.conv2d_f32(x.to(dev), ops.pack_conv_weight(w.to(dev)), ksize, upsample=ups, bias=b.to(dev), residual=r.to(dev), algo=algo, wu=None)
    return y.cpu(), None


def test_out_must_be_the_output_itself(dev):
    x, w = torch.zeros(1, 4, 4, 32, device=dev), torch.zeros(8, 288, device=dev)
    for bad in (torch.empty(1, 4, 4, 4, device=dev), torch.empty(1, 4, 4, 8, device=dev, dtype=torch.float16),
                torch.empty(1, 4, 4, 16, device=dev)[..., :8]):
        with pytest.raises(AssertionError):
            ops.conv2d_f32(x, w, 3, algo="direct", out=bad)
