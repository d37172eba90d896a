"""EfficientViT-SAM image encoder on the HIP kernels (-m gpu): the three new kernels against torch fp32 on the same 16-bit operands,
the narrow encoder against the fixture of the reference's own classes (tests/golden/effvit_golden.npz), batch invariance, and the
full-width l0 against a per-layer fallback.

Kernel tolerances are measured, not chosen: for every case the same computation is done by torch on the GPU in the storage dtype, its
error E against the fp32 result is taken, and the HIP kernel is allowed 2 E (another accumulation order) plus one ulp of the storage
dtype at the output's largest magnitude.  With OMG_EFFVIT_ERRORS_JSON=path the measured values are written there when the module is
done."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from omg_amd import ops
from omg_amd.efficientvit import EfficientViTSamImageEncoder
from tests.effvit_torch import TorchEncoder, build_from_fixture, load_fixture, seed_encoder

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "effvit_golden.npz")
DTYPES = [torch.float16, torch.bfloat16]
SIZES = [(7, 9), (32, 32)]
MEASURED = {}
CANARY = 1234.0


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("OMG_EFFVIT_ERRORS_JSON")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def fixture():
    return load_fixture(GOLD)


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float16):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def ulp(dtype, mag):
    bits = 10 if dtype == torch.float16 else 7
    return 2.0 ** (math.floor(math.log2(max(mag, 2.0 ** -14))) - bits)


def gelu(x):
    return F.gelu(x, approximate="tanh")


def check(tag, dtype, got, ref32, torch16):
    """got, torch16: results in the storage dtype (NCHW, on any device); ref32: fp32 on the CPU."""
    e_torch = (torch16.float().cpu() - ref32).abs().max().item()
    e_hip = (got.float().cpu() - ref32).abs().max().item()
    bound = 2.0 * e_torch + ulp(dtype, ref32.abs().max().item())
    MEASURED[tag] = {"torch_storage_dtype_err": e_torch, "hip_err": e_hip, "bound": bound, "max_abs_ref": ref32.abs().max().item()}
    print(f"{tag}: hip {e_hip:.3e}  torch-{str(dtype)[6:]} {e_torch:.3e}  bound {bound:.3e}")
    assert e_hip <= bound, (tag, e_hip, bound)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def with_canary(shape, row_elems, dtype, dev):
    """A contiguous output view of ``shape`` in front of one extra image row of canary values."""
    n = math.prod(shape)
    flat = torch.full((n + row_elems,), CANARY, dtype=dtype, device=dev)
    return flat, flat[:n].view(shape)


# ------------------------------------------------------------------------------------------------ kernel 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cout", [32, 64, 80])
@pytest.mark.parametrize("cin", [3, 32, 96, 128])
def test_conv3x3_nhwc_act(dev, dtype, cin, cout):
    """Cin 3 (element loads, K padded in the kernel), 32 / 96 (no multiple of 64), 128; Cout 32 / 64 / 80 = the three tile widths, 80 with a
    partial last tile; 7 x 9 puts the stride-2 last row and column on the padding, 2 x 32 x 32 is more than one block."""
    B = 2
    with torch.backends.cudnn.flags(enabled=False):
        for (H, W) in SIZES:
            x = rnd(B, cin, H, W, seed=1, dtype=dtype)
            w = rnd(cout, cin, 3, 3, seed=2, scale=(1.0 / (9 * cin)) ** 0.5, dtype=dtype)
            b = rnd(cout, seed=3, scale=0.5, dtype=dtype)
            xd, wd, bd = nhwc(x).to(dev), nhwc(w).to(dev), b.to(dev)
            for stride in (1, 2):
                Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
                r = rnd(B, cout, Ho, Wo, seed=4, dtype=dtype)
                pre32 = F.conv2d(x.float(), w.float(), b.float(), stride=stride, padding=1)
                pre16 = F.conv2d(x.to(dev), w.to(dev), bd, stride=stride, padding=1)
                assert pre32.shape == (B, cout, Ho, Wo)
                for act in (False, True):
                    for res in (False, True):
                        ref32 = (gelu(pre32) if act else pre32) + (r.float() if res else 0.0)
                        t16 = gelu(pre16) if act else pre16
                        t16 = t16 + r.to(dev) if res else t16
                        flat, out = with_canary((B, Ho, Wo, cout), Wo * cout, dtype, dev)
                        got = ops.conv3x3_nhwc_act(xd, wd, stride=stride, bias=bd, gelu=act, residual=nhwc(r).to(dev) if res else None, out=out)
                        assert torch.all(flat[out.numel():] == CANARY), "wrote past the output"
                        check(f"conv3x3 {str(dtype)[6:]} cin{cin} cout{cout} {H}x{W} s{stride} gelu{int(act)} res{int(res)}", dtype,
                              got.permute(0, 3, 1, 2), ref32, t16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,stride", [(3, 32, 2), (32, 80, 1), (96, 64, 2), (128, 32, 1)])
def test_conv3x3_exact_on_small_integers(dev, dtype, cin, cout, stride):
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 7, 9
    x = torch.randint(-1, 2, (B, cin, H, W), generator=g).float()
    w = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float() * (torch.rand(cout, cin, 3, 3, generator=g) < 0.25)
    b = torch.randint(-4, 5, (cout,), generator=g).float()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = torch.randint(-4, 5, (B, cout, Ho, Wo), generator=g).float()
    ref = F.conv2d(x, w, b, stride=stride, padding=1) + r
    assert torch.equal(ref, ref.to(dtype).float()) and ref.abs().max() >= 8, "the case itself must be exactly representable"
    got = ops.conv3x3_nhwc_act(nhwc(x).to(dtype).to(dev), nhwc(w).to(dtype).to(dev), stride=stride, bias=b.to(dtype).to(dev),
                               residual=nhwc(r).to(dtype).to(dev))
    assert torch.equal(got.permute(0, 3, 1, 2).float().cpu(), ref)


# ------------------------------------------------------------------------------------------------ kernel 2
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24, 256])
def test_dwconv3x3_act(dev, dtype, C):
    B = 2
    with torch.backends.cudnn.flags(enabled=False):
        for (H, W) in SIZES:
            x = rnd(B, C, H, W, seed=6, dtype=dtype)
            w = rnd(C, 1, 3, 3, seed=7, scale=1.0 / 3, dtype=dtype)
            b = rnd(C, seed=8, scale=0.5, dtype=dtype)
            wide = torch.full((B * H * W, C + 16), 7.0, dtype=dtype)              # the kernel takes a row stride: a column slice of a wider buffer
            wide[:, 8:8 + C] = nhwc(x).reshape(-1, C)
            xd = wide.to(dev)[:, 8:8 + C]
            taps, bd = w.reshape(C, 9).t().contiguous().to(dev), b.to(dev)
            for stride in (1, 2):
                Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
                for act_out in (False, True):
                    for act_in in (False, True):
                        xin32, xin16 = (gelu(x.float()), gelu(x.to(dev))) if act_in else (x.float(), x.to(dev))
                        ref32 = F.conv2d(xin32, w.float(), b.float(), stride=stride, padding=1, groups=C)
                        t16 = F.conv2d(xin16, w.to(dev), bd, stride=stride, padding=1, groups=C)
                        if act_out:
                            ref32, t16 = gelu(ref32), gelu(t16)
                        got = ops.dwconv3x3_act(xd, taps, B, H, W, stride=stride, bias=bd, gelu=act_out, gelu_in=act_in)
                        assert got.shape == (B * Ho * Wo, C)
                        check(f"dwconv3x3 {str(dtype)[6:]} c{C} {H}x{W} s{stride} gelu{int(act_out)} gelu_in{int(act_in)}", dtype,
                              got.view(B, Ho, Wo, C).permute(0, 3, 1, 2), ref32, t16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,stride", [(8, 1), (24, 2), (256, 2)])
def test_dwconv3x3_exact_on_small_integers(dev, dtype, C, stride):
    g = torch.Generator().manual_seed(9)
    B, H, W = 2, 7, 9
    x = torch.randint(-3, 4, (B, C, H, W), generator=g).float()
    w = torch.randint(-2, 3, (C, 1, 3, 3), generator=g).float()
    b = torch.randint(-4, 5, (C,), generator=g).float()
    ref = F.conv2d(x, w, b, stride=stride, padding=1, groups=C)
    assert torch.equal(ref, ref.to(dtype).float()) and ref.abs().max() >= 8
    got = ops.dwconv3x3_act(nhwc(x).reshape(-1, C).to(dtype).to(dev), w.reshape(C, 9).t().contiguous().to(dtype).to(dev), B, H, W, stride=stride,
                            bias=b.to(dtype).to(dev))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert torch.equal(got.view(B, Ho, Wo, C).permute(0, 3, 1, 2).float().cpu(), ref)


# ------------------------------------------------------------------------------------------------ kernel 3
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hin,win,hout,wout", [(8, 8, 64, 64), (16, 16, 64, 64), (32, 32, 64, 64), (5, 7, 10, 14)])
def test_upsample_add_nhwc(dev, dtype, hin, win, hout, wout):
    B, C = 2, 24
    x = rnd(B, C, hin, win, seed=10, dtype=dtype)
    y0 = rnd(B, C, hout, wout, seed=11, dtype=dtype)
    up32 = F.interpolate(x.float(), size=(hout, wout), mode="bicubic", align_corners=False)
    up16 = F.interpolate(x.to(dev), size=(hout, wout), mode="bicubic", align_corners=False)
    for accumulate in (True, False):
        ref32 = up32 + y0.float() if accumulate else up32
        t16 = up16 + y0.to(dev) if accumulate else up16
        flat, out = with_canary((B, hout, wout, C), wout * C, dtype, dev)
        out.copy_(nhwc(y0).to(dev))
        ops.upsample_add_nhwc(nhwc(x).to(dev), out, accumulate=accumulate)
        assert torch.all(flat[out.numel():] == CANARY), "wrote past the output"
        check(f"upsample_add {str(dtype)[6:]} {hin}x{win}->{hout}x{wout} acc{int(accumulate)}", dtype, out.permute(0, 3, 1, 2), ref32, t16)


# ------------------------------------------------------------------------------------------------ the encoder
BASE = {torch.float16: 3e-2, torch.bfloat16: 2e-1}          # tests/test_litemla_gpu.py: max |d| / rms against the golden vectors, one block


def depths(cfg):
    """Blocks in front of each checked tensor (a LiteMLA module = 1, as in its own test): the stem and every ResBlock / FusedMBConv /
    MBConv / LiteMLA count one each, the neck's fusion, its output convolution and the LayerNorm one each.  Rounding errors of
    successive blocks are independent, so the bound grows with the square root of the depth."""
    d, n = {}, 1
    for s, dep in enumerate(cfg.depth_list):
        n += (1 if s else 0) + dep * (2 if cfg.block_list[s] == "att" else 1)
        d[f"stage{s}"] = n
    d["neck_mid"] = n + 1 + cfg.head_depth
    d["neck"] = d["neck_mid"] + 1
    d["out"] = d["neck"] + 1
    return d


@pytest.mark.parametrize("dtype", DTYPES)
def test_narrow_encoder_matches_the_reference_classes(dev, dtype, fixture):
    _, cfg, sd, vec, sub = fixture
    m = build_from_fixture(cfg, sd, dtype, dev)
    feats = m.forward_features(vec["x"].to(dtype).to(dev))
    emb = m(vec["x"].to(dtype).to(dev))
    assert emb.shape == (1, 256, 64, 64) and torch.equal(emb, feats["out"].permute(0, 3, 1, 2))
    dep = depths(cfg)
    failed = []
    for k, d in dep.items():
        got = feats[k].permute(0, 3, 1, 2).float().cpu()
        if k in ("neck", "out"):
            got = got[:, :, ::sub, ::sub]
        ref = vec[k]
        assert got.shape == ref.shape and torch.isfinite(got).all(), k
        rel = (got - ref).abs().max().item() / ref.pow(2).mean().sqrt().item()
        bound = BASE[dtype] * math.sqrt(d)
        MEASURED[f"encoder {str(dtype)[6:]} {k}"] = {"rel_err_max_over_rms": rel, "depth": d, "bound": bound}
        print(f"narrow encoder {dtype} {k}: max |d| / rms {rel:.3e}  (depth {d}, bound {bound:.3e})")
        if not rel < bound:
            failed.append((k, rel, bound))
    assert not failed, failed


def test_batch_invariance(dev, fixture):
    _, cfg, sd, _, _ = fixture
    m = build_from_fixture(cfg, sd, torch.float16, dev)
    x = rnd(3, 3, 128, 128, seed=12).to(dev)
    together = m(x)
    for i in range(3):
        assert torch.equal(m(x[i:i + 1]), together[i:i + 1]), f"image {i} differs alone and in a batch of 3"


def test_full_width_l0_against_the_per_layer_fallback(dev):
    """l0 at its real size: finite, [1, 256, 64, 64], and equal to the per-layer fallback (every convolution F.conv2d in fp16 on the GPU,
    LiteMLA as the module) within the accumulated-rounding bound of the narrow model's form: BASE sqrt(depth), times sqrt(2) as BOTH
    sides carry their own 16-bit rounding of every layer."""
    dt = torch.float16
    m = EfficientViTSamImageEncoder("l0", dtype=dt, device=dev)
    seed_encoder(m, 30)
    x = rnd(1, 3, 512, 512, seed=13).to(dev)
    got = m(x)
    assert got.shape == (1, 256, 64, 64) and got.dtype == dt and torch.isfinite(got).all()
    with torch.backends.cudnn.flags(enabled=False):
        ref = TorchEncoder(m, rounded=True).features(x)["out"]
    assert torch.isfinite(ref).all()
    rel = (got.float() - ref.float()).abs().max().item() / ref.float().pow(2).mean().sqrt().item()
    d = depths(m.cfg)["out"]
    bound = BASE[dt] * math.sqrt(2 * d)
    MEASURED["encoder l0 512 float16 out vs per-layer fallback"] = {"rel_err_max_over_rms": rel, "depth": d, "bound": bound}
    print(f"l0 512x512 fp16: max |d| / rms vs the per-layer fallback {rel:.3e}  (depth {d}, bound {bound:.3e})")
    assert rel < bound
