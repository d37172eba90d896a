"""conv_f32_wino_kernel (csrc/conv_f32_wino.hip): the fp32 3x3 convolution of the upcast VAE decode as Winograd F(2x2, 3x3).
Reference everywhere: a float64 convolution on the CPU (never the other kernel).  Bound: 2e-5, the project's bound for this op
(test_fp32_kernels_match_torch_fp32); an fp32 emulation of F(2x2, 3x3) on these shapes stays <= 4.6e-6."""
import pytest
import torch
import torch.nn.functional as F

from omg_amd import ops
from omg_amd.vae import AutoencoderKLDecoder, VaeConfig
from oracle import vae as ov

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, Cout, ksize, upsample): the four cases of test_fp32_kernels_match_torch_fp32, the VAE's own channel counts, a non-square one
CASES = [(2, 16, 16, 128, 128, 3, False), (1, 24, 24, 256, 128, 3, True), (2, 20, 20, 64, 96, 1, False), (1, 33, 33, 32, 260, 3, False),
         (1, 32, 32, 512, 512, 3, False), (1, 64, 64, 256, 256, 3, False), (1, 16, 16, 512, 512, 3, True), (2, 24, 16, 128, 256, 3, False)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _case(g, B, H, W, Cin, Cout, k, ups):
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (k * k * Cin) ** -0.5
    b = torch.randn(Cout, generator=g)
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    res = torch.randn(B, Ho, Wo, Cout, generator=g)
    xin = x.permute(0, 3, 1, 2)
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin.double(), w.double(), b.double(), padding=k // 2).permute(0, 2, 3, 1) + res.double()
    return x, w, b, res, ref


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_winograd_and_direct_match_float64(dev, case):
    """Both kernels against the float64 convolution, with bias and residual, so that a failure says which kernel moved.  The 1x1 and the
    odd-sized case have no F(2x2, 3x3) form: there algo="winograd" must refuse and algo="auto" must launch the direct kernel."""
    B, H, W, Cin, Cout, k, ups = case
    x, w, b, res, ref = _case(torch.Generator().manual_seed(0), *case)
    xd, wd, bd, rd = x.to(dev), ops.pack_conv_weight(w.to(dev)), b.to(dev), res.to(dev)
    y = ops.conv2d_f32(xd, wd, k, upsample=ups, bias=bd, residual=rd, algo="direct")
    assert ops.LAST_CONV2D_F32_ALGO == "direct"
    e_direct = (y.cpu().double() - ref).abs().max().item()
    print(f"{case}: direct max|err| {e_direct:.2e}")
    eligible = k == 3 and H % 2 == 0 and W % 2 == 0 or (k == 3 and ups)
    if eligible:
        wu = ops.pack_conv_weight_wino(w.to(dev))
        y = ops.conv2d_f32(xd, wd, k, upsample=ups, bias=bd, residual=rd, algo="winograd", wu=wu)
        assert ops.LAST_CONV2D_F32_ALGO == "winograd"
        e_wino = (y.cpu().double() - ref).abs().max().item()
        print(f"{case}: winograd max|err| {e_wino:.2e}")
        assert e_wino < 2e-5, (case, "winograd", e_wino)
    else:
        wu = ops.pack_conv_weight_wino(w.to(dev)) if k == 3 else None
        with pytest.raises(Exception):
            ops.conv2d_f32(xd, wd, k, upsample=ups, bias=bd, residual=rd, algo="winograd", wu=wu)
        ops.set_conv2d_f32_auto(True, 0)
        try:
            y = ops.conv2d_f32(xd, wd, k, upsample=ups, bias=bd, residual=rd, algo="auto", wu=wu)
        finally:
            ops.set_conv2d_f32_auto()
        assert ops.LAST_CONV2D_F32_ALGO == "direct"
        assert (y.cpu().double() - ref).abs().max().item() < 2e-5
    assert e_direct < 2e-5, (case, "direct", e_direct)


def test_auto_takes_winograd_only_where_the_launch_fills_the_machine(dev):
    g = torch.Generator().manual_seed(3)
    for (B, H, Cin, Cout, want) in [(1, 16, 32, 64, "direct"), (1, 256, 32, 64, "winograd")]:
        x = torch.randn(B, H, H, Cin, generator=g).to(dev)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).to(dev)
        prof = ops.KernelProfiler()
        ops.set_profiler(prof)
        try:
            y = ops.conv2d_f32(x, ops.pack_conv_weight(w), 3, wu=ops.pack_conv_weight_wino(w))
        finally:
            ops.set_profiler(None)
        assert ops.LAST_CONV2D_F32_ALGO == want
        (kind, flops, _, _, tag), = prof.records
        assert kind == "gemm_f32" and tag[0] == ("conv_f32_wino" if want == "winograd" else "conv_f32")
        direct_flops = 2.0 * B * H * H * Cout * 9 * Cin
        assert flops == (direct_flops * 16 / 36 if want == "winograd" else direct_flops)      # the EXECUTED matrix FLOPs
        ref = F.conv2d(x.cpu().permute(0, 3, 1, 2).double(), w.cpu().double(), padding=1).permute(0, 2, 3, 1)
        assert (y.cpu().double() - ref).abs().max().item() < 2e-5


def test_winograd_addresses_beyond_32_bits(dev):
    """The 5.4 GB input of test_fp32_conv_addresses_beyond_32_bits_and_tiles_across_images through the Winograd kernel (32-bit lane offsets
    from the block's own image), on sampled output pixels against a float64 dot product."""
    g = torch.Generator().manual_seed(1)
    B, H, Cin, Cout = 5, 1024, 256, 128
    gd = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(B, H, H, Cin, generator=gd, device=dev)
    assert x.numel() * 4 > 4 * 2 ** 30
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    y = ops.conv2d_f32(x, ops.pack_conv_weight(w.to(dev)), 3, algo="winograd", wu=ops.pack_conv_weight_wino(w.to(dev)))
    pts = [(0, 0, 0), (0, H - 1, H - 1), (1, 0, 0), (2, 511, 513), (3, H - 1, 0), (4, 0, H - 1), (4, 777, 3), (4, H - 1, H - 1), (4, H - 2, H - 2)]
    pts += [(int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, H, (1,), generator=g))) for _ in range(24)]
    wd = w.double()
    for (bi, yy, xx) in pts:
        acc = torch.zeros(Cout, dtype=torch.float64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                iy, ix = yy + dy, xx + dx
                if 0 <= iy < H and 0 <= ix < H:
                    acc += wd[:, :, dy + 1, dx + 1] @ x[bi, iy, ix].cpu().double()
        err = (y[bi, yy, xx].cpu().double() - acc).abs().max().item()
        assert err < 2e-5, (bi, yy, xx, err)
    del x, y
    torch.cuda.empty_cache()


def test_upcast_decode_winograd_against_the_oracle_and_deterministic(dev):
    """Reduced-width upcast decode: the error of the Winograd path against the decode oracle must be <= 3x the error of the direct path
    against the same oracle (a per-convolution fp32 emulation shows up to 2.6x); both values are printed.  decode_latents stays
    deterministic on the new path."""
    cfg_o, cfg_p = ov.VaeConfig.tiny(), VaeConfig.tiny()
    sd = ov.init_state_dict(cfg_o, seed=4)
    vae = AutoencoderKLDecoder(cfg_p, dtype=torch.float16, device=dev, upcast=True)
    vae.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    sd_r = {k: (v.half().float() if k.startswith(("decoder.conv_in", "decoder.mid_block")) else v) for k, v in sd.items()}
    z = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(5))
    ref = ov.decode(sd_r, cfg_o, z).double()
    rms = ref.pow(2).mean().sqrt()
    errs = {}
    try:
        for name, on in (("direct", False), ("winograd", True)):
            ops.set_conv2d_f32_auto(on, 0)
            out = vae.decode(z.to(dev))
            errs[name] = ((out.double().cpu() - ref).pow(2).mean().sqrt() / rms).item()
        assert vae.decoder.up_blocks[0].resnets[0].conv1.wino_weight() is not None
        lat = z.to(dev) * cfg_p.scaling_factor
        assert torch.equal(vae.decode_latents(lat), vae.decode_latents(lat))
    finally:
        ops.set_conv2d_f32_auto()
    print(f"upcast decode (tiny) rms err vs oracle: direct {errs['direct']:.3e}, winograd {errs['winograd']:.3e}")
    assert errs["winograd"] <= 3 * errs["direct"], errs
