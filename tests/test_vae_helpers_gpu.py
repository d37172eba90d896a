"""The small kernels around the fp32 convolutions of the upcast VAE decode (csrc/misc.hip): softmax_rows_kernel, channel_mix_kernel,
cast_f32_kernel and the fp32 conv_out_kernel, at the sizes where their loops and reductions change shape.  References are float64 on the
CPU; every tolerance is an exact comparison or a rounding bound written out where it is used."""
import pytest
import torch
import torch.nn.functional as F

from omg_amd import ops
from tests import _conv_f32_model as M

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
COLS = [1, 2, 255, 256, 257, 1000, 16384]          # one thread, one wave's worth, one under / at / over one pass of the 256 threads, several passes
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _name(dtype):
    return "fp16" if dtype == torch.float16 else "bf16"


def _softmax(dev, x16, cols, ld, scale):
    """softmax_rows_ on the first ``cols`` columns of a [rows, ld] buffer whose pad columns hold a marker -> (result, pad) on the CPU."""
    buf = torch.full((x16.shape[0], ld), 7.0, dtype=x16.dtype)
    buf[:, :cols] = x16
    d = buf.to(dev)
    out = ops.softmax_rows_(d[:, :cols], scale)
    assert out.data_ptr() == d.data_ptr()
    d = d.cpu()
    return d[:, :cols], d[:, cols:]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", COLS)
def test_softmax_rows_inside_its_rounding_bound(dev, dtype, rows, cols):
    """|out - p| <= u16 p + (cols / 256 + 8) 2^-23 p (+ 2^-25 for fp16), p the float64 softmax of the stored scores times float32(scale):
    derived in tests/_conv_f32_model.py, held by the fp32 emulation there (tests/test_conv_f32_model.py)."""
    g = torch.Generator().manual_seed(cols * 8 + rows)
    x = (torch.randn(rows, cols, generator=g) * 3).to(dtype)
    for (ld, scale) in ((cols, 1.0), (cols + 24, 0.37)):
        out, pad = _softmax(dev, x, cols, ld, scale)
        assert bool((pad == 7.0).all()), "pad columns written"
        p = M.softmax_truth(x, scale)
        err, tol = (out.double() - p).abs(), M.softmax_bound(p, cols, dtype)
        print(f"RATIO softmax {_name(dtype)} {rows}x{cols} ld {ld}: worst err / bound {(err / tol).max().item():.4f}")
        assert bool((err <= tol).all()), (rows, cols, ld, (err / tol).max().item())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("cols", COLS)
def test_softmax_rows_exact_cases(dev, dtype, cols):
    # all scores equal, score and scale powers of two (or 0): x * sl2 and ml2 are the same exact product, every exponential is exp2(0) = 1,
    # the sum is cols exactly and the result 1 / cols, rounded to fp32 by the reciprocal and once more at the store.  The two roundings
    # equal one here: fp32(1 / cols) and its two neighbours round to the same 16-bit value (asserted, so that the claim is not luck)
    inv = torch.tensor(1.0 / cols, dtype=torch.float32)
    want = torch.tensor(1.0 / cols, dtype=torch.float64).to(dtype)
    for nb in (inv, torch.nextafter(inv, torch.tensor(0.0)), torch.nextafter(inv, torch.tensor(1.0))):
        assert nb.to(dtype) == want
    for (v, scale) in ((0.0, 0.37), (2.0, 0.5), (-4.0, 1.0), (1024.0, 0.125)):
        out, pad = _softmax(dev, torch.full((5, cols), v, dtype=dtype), cols, cols + 8, scale)
        assert torch.equal(out, want.expand(5, cols)), (cols, v, scale)
        assert bool((pad == 7.0).all())
    # one score 200 above the rest: exp(-200) is 0 in every format here, the result exactly one 1 and zeros
    x = torch.randn(5, cols, generator=torch.Generator().manual_seed(cols)).to(dtype)
    hot = torch.arange(5) * 37 % cols
    x[torch.arange(5), hot] = 204.0
    out, _ = _softmax(dev, x, cols, cols, 1.0)
    want = torch.zeros(5, cols, dtype=dtype)
    want[torch.arange(5), hot] = 1.0
    assert torch.equal(out, want), cols


@pytest.mark.parametrize("cols", COLS)
def test_softmax_rows_fp16_scores_at_the_edge_of_the_format(dev, cols):
    """Scores of +-60000 with the decode's scale 512^-0.5: the scaled differences reach 5300, nothing may overflow on the way: finite, and
    each row sums to 1 within the sum of the elementwise bounds."""
    g = torch.Generator().manual_seed(cols)
    x = torch.where(torch.rand(5, cols, generator=g) < 0.5, 60000.0, -60000.0).to(torch.float16)
    x[1] = -60000.0                                  # a row whose maximum is the most negative score
    x[2, 0] = 60000.0
    out, _ = _softmax(dev, x, cols, cols, 512 ** -0.5)
    assert bool(torch.isfinite(out).all())
    p = M.softmax_truth(x, 512 ** -0.5)
    tol = M.softmax_bound(p, cols, torch.float16).sum(dim=-1)
    assert bool(((out.double().sum(dim=-1) - 1.0).abs() <= tol).all()), (out.double().sum(dim=-1), tol)
    assert bool(((out.double() - p).abs() <= M.softmax_bound(p, cols, torch.float16)).all())


# (B, Cin, Cout, HW, bias): every (Cin, Cout) of {1, 3, 4, 8}^2 at HW = 257 (one block and one thread), bias alternating; HW = 1 and 255
# (less than a block); 1024 * 256 + 5 = 5 pixels more than the capped grid covers at once, the grid-stride loop's second turn
MIX_CASES = [(3 if (ci + co) % 2 else 1, ci, co, 257, (ci * co) % 2 == 0) for ci in (1, 3, 4, 8) for co in (1, 3, 4, 8)]
MIX_CASES += [(1, 4, 4, 1, True), (3, 8, 3, 1, False), (3, 4, 8, 255, True), (1, 3, 1, 255, False),
              (1, 8, 8, 1024 * 256 + 5, True), (3, 3, 4, 1024 * 256 + 5, False)]


@pytest.mark.parametrize("case", MIX_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_channel_mix_exact_on_integers_and_inside_the_fma_chain_bound(dev, case):
    """out = bias + sum_c w x by Cin fmas from the bias: Cin roundings of partial sums bounded by S = |w| |x| + |bias|, so
    |err| <= (Cin + 1) 2^-24 S to first order with one to spare; integers are exact."""
    B, Cin, Cout, HW, bias = case
    g = torch.Generator().manual_seed(Cin * 8 + Cout)
    Hh, Ww = 1, HW
    for kind in ("int", "randn"):
        if kind == "int":
            x = torch.randint(-9, 10, (B, Cin, Hh, Ww), generator=g).float()
            w = torch.randint(-9, 10, (Cout, Cin), generator=g).float()
            b = torch.randint(-9, 10, (Cout,), generator=g).float()
        else:
            x, w, b = torch.randn(B, Cin, Hh, Ww, generator=g) + 0.5, torch.randn(Cout, Cin, generator=g), torch.randn(Cout, generator=g)
        y = ops.channel_mix(x.to(dev), w.to(dev), b.to(dev) if bias else None).cpu()
        assert y.shape == (B, Cout, Hh, Ww)
        ref = torch.einsum("oc,bchw->bohw", w.double(), x.double())
        S = torch.einsum("oc,bchw->bohw", w.double().abs(), x.double().abs())
        if bias:
            ref, S = ref + b.double().view(1, -1, 1, 1), S + b.double().abs().view(1, -1, 1, 1)
        if kind == "int":
            assert torch.equal(y.double(), ref), case
        else:
            err, tol = (y.double() - ref).abs(), (Cin + 1) * U24 * S
            print(f"RATIO channel_mix {case}: worst err / bound {(err / tol).max().item():.4f}")
            assert bool((err <= tol).all()), (case, (err / tol).max().item())


def _same_bits_nan_as_nan(got, want):
    """fp32 tensors: equal bit for bit wherever ``want`` is a number, NaN wherever it is NaN."""
    nan = torch.isnan(want)
    return bool((torch.isnan(got) == nan).all()) and bool((got.view(torch.int32) == want.view(torch.int32))[~nan].all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_cast_f32_on_every_bit_pattern(dev, dtype):
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    assert x.view(torch.int16).unique().numel() == 65536
    y = ops.cast_f32(x.to(dev)).cpu()
    assert y.dtype == torch.float32 and _same_bits_nan_as_nan(y, x.float())
    assert bool((torch.signbit(y) == torch.signbit(x.float())).all())          # -0, -inf and the sign of every number


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_cast_f32_beyond_the_block_cap(dev, dtype):
    """16384 blocks x 256 threads x 8 elements is one pass of the capped grid: 300 vectors more run the grid-stride loop's second turn."""
    n = 16384 * 256 * 8 + 8 * 300
    x = torch.randint(0, 65536, (n,), dtype=torch.int32, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(torch.int16).view(dtype)
    y = ops.cast_f32(x)
    want = x.float()
    assert y.shape == want.shape and _same_bits_nan_as_nan(y, want)             # every element, compared on the device
    xc = x.cpu()
    idx = torch.cat((torch.arange(n - 8 * 300 - 64, n), torch.arange(0, n, 65521)))        # the second turn, the seam before it and a sample
    assert _same_bits_nan_as_nan(y.cpu()[idx], xc[idx].float())
    del x, y, want
    torch.cuda.empty_cache()


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("bhw", [(1, 1, 1), (2, 5, 7)], ids=str)
@pytest.mark.parametrize("cin", [8, 128])
@pytest.mark.parametrize("cout", [1, 3, 8])
def test_fp32_conv_out_exact_on_integers_and_inside_its_bound(dev, cout, cin, bhw, bias):
    """A wave per pixel: each lane adds its share of the 9 Cin products, six shuffles add the lanes, then the bias: fewer than 9 Cin + 2
    roundings of partial sums bounded by S = conv(|x|, |w|) + |bias| on any path, so |err| <= (9 Cin + 2) 2^-24 S; integers are exact."""
    B, H, W = bhw
    g = torch.Generator().manual_seed(cout * 1000 + cin)
    for kind in ("int", "randn"):
        if kind == "int":
            x = torch.randint(-3, 4, (B, H, W, cin), generator=g).float()
            w = torch.randint(-8, 9, (cout, cin, 3, 3), generator=g).float()
            b = torch.randint(-8, 9, (cout,), generator=g).float()
        else:
            x, w, b = torch.randn(B, H, W, cin, generator=g) + 0.5, torch.randn(cout, cin, 3, 3, generator=g) * 0.03, torch.randn(cout, generator=g)
        out = torch.full((B * cout * H * W + 64,), -7.5, device=dev)
        y = ops.conv_out(x.to(dev), w.permute(0, 2, 3, 1).contiguous().to(dev), b.to(dev) if bias else None,
                         out=out[:B * cout * H * W].view(B, cout, H, W)).cpu()
        assert bool((out[B * cout * H * W:] == -7.5).all())
        xin = x.permute(0, 3, 1, 2).double()
        ref = F.conv2d(xin, w.double(), b.double() if bias else None, padding=1)
        S = F.conv2d(xin.abs(), w.double().abs(), b.double().abs() if bias else None, padding=1)
        if kind == "int":
            assert torch.equal(y.double(), ref), (cout, cin, bhw, bias)
        else:
            err, tol = (y.double() - ref).abs(), (9 * cin + 2) * U24 * S
            print(f"RATIO conv_out {cout}x{cin} {bhw} bias {bias}: worst err / bound {(err / tol).max().item():.4f}")
            assert bool((err <= tol).all()), (cout, cin, bhw, bias, (err / tol).max().item())
