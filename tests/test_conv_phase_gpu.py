"""The phase form of the nearest-2x upsample + 3x3 convolution on the GPU (-m gpu): ``ops.conv2d(upsample=2)`` — four 2x2 convolutions on the
source image, gemm_phase_kernel (128x128) and gemm_phase_kernel_v13 (256x320) — against the direct form ``upsample=True`` and a float64 reference.
DESIGN §5 "The upsample convolution: four 2x2 phases"."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from omg_amd.modules import Conv2d

# the project's kernel tolerance (tests/test_kernels_gpu.py)
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}
# the module tolerance of tests/test_unet_gpu.py
TOL_UNET = {torch.float16: 3e-2, torch.bfloat16: 2e-1}


def phase_w(w_oihw):
    return ops.pack_conv_weight_phase(w_oihw)


def forced(variant):
    """Context manager: the GEMM tile variant forced through the debug hook (1 = the 128x128 kernel, 28 = the 256x320 tile, 0 = the chooser)."""
    class _F:
        def __enter__(self):
            L.lib().omg_debug_set_gemm_variant(variant)

        def __exit__(self, *a):
            L.lib().omg_debug_set_gemm_variant(0)
    return _F()


# ------------------------------------------------------------------ exact: taps, padding, phase order, output scatter
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (1, 6), (5, 7), (16, 16)])
@pytest.mark.parametrize("cout", [8, 320, 328])
def test_phase_form_equals_the_direct_form_where_every_sum_is_exact(dev, B, hw, cout):
    """Integer inputs in [-2, 2], weights in {-1, 0, 1}, Cin = 64: every product, every partial sum (|y| <= 2 * 9 * 64) and every summed phase
    weight (|w| <= 4) is an integer fp16 holds exactly, so both forms must give the same bits on both kernels — independent of rounding."""
    H, W = hw
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W * 10 + cout)
    x = torch.randint(-2, 3, (B, H, W, 64), generator=g).to(torch.float16).to(dev)
    w = torch.randint(-1, 2, (cout, 64, 3, 3), generator=g).to(torch.float16).to(dev)
    with forced(1):
        want = ops.conv2d(x, ops.pack_conv_weight(w), 3, upsample=True)
    ref = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2).double().cpu(), scale_factor=2, mode="nearest"), w.double().cpu(), padding=1).permute(0, 2, 3, 1)
    assert ref.abs().max().item() <= 2048 and torch.equal(want.double().cpu(), ref)      # the direct form is itself exact here
    wp = phase_w(w)
    for v in (0, 1, 28):
        with forced(v):
            got = ops.conv2d(x, wp, 3, upsample=2)
        assert got.shape == want.shape == (B, 2 * H, 2 * W, cout)
        assert torch.equal(got, want), f"variant {v}: {(got.float() - want.float()).abs().max().item()}"


# ------------------------------------------------------------------ rounding: both forms against float64
_ROUND_CASES = {}


def rounding_case(dev, dtype, cin, B=2, H=5, W=7, cout=72):
    """Inputs (rounded to ``dtype``), the float64 reference and both forms' results of one case; computed once and shared."""
    key = (dtype, cin, B, H, W, cout)
    if key not in _ROUND_CASES:
        g = torch.Generator().manual_seed(cin + B * 7 + H)
        x = torch.randn(B, H, W, cin, generator=g).to(dtype)
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).to(dtype)
        bias = torch.randn(cout, generator=g).to(dtype)
        gb = torch.randn(B, cout, generator=g).to(dtype)
        ref = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2, mode="nearest"), w.double(), padding=1).permute(0, 2, 3, 1)
        ref = ref + bias.double() + gb.double()[:, None, None, :]
        xd, wd, bd, gd = x.to(dev), w.to(dev), bias.to(dev), gb.to(dev)
        with forced(1):
            direct = ops.conv2d(xd, ops.pack_conv_weight(wd), 3, upsample=True, bias=bd, group_bias=gd)
            phase = ops.conv2d(xd, phase_w(wd), 3, upsample=2, bias=bd, group_bias=gd)
        _ROUND_CASES[key] = dict(x=xd, w=wd, bias=bd, gb=gd, ref=ref, direct=direct, phase=phase)
    return _ROUND_CASES[key]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin", [64, 192, 1280])
def test_phase_form_against_float64_at_the_kernel_tolerance(dev, dtype, cin):
    """N(0, 1) data, bias and per-sample bias on, M = 2 * 5 * 7 = 70 rows per phase (no multiple of 256: ragged tiles, per-row group bias)."""
    c = rounding_case(dev, dtype, cin)
    ref = c["ref"]
    for name in ("direct", "phase"):
        e = (c[name].double().cpu() - ref).abs()
        print(f"{dtype} cin={cin} {name}: rms err {e.pow(2).mean().sqrt().item():.3e} max err {e.max().item():.3e} "
              f"worst err/tol {(e / (TOL[dtype] + TOL[dtype] * ref.abs())).max().item():.3f}")
    torch.testing.assert_close(c["phase"].double().cpu(), ref, rtol=TOL[dtype], atol=TOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_phase_form_with_the_folded_per_sample_bias(dev, dtype):
    """16 x 16 source pixels = 256 rows per sample: the per-sample bias starts the accumulators (the rule every variant shares)."""
    c = rounding_case(dev, dtype, 64, B=3, H=16, W=16, cout=320)
    torch.testing.assert_close(c["phase"].double().cpu(), c["ref"], rtol=TOL[dtype], atol=TOL[dtype])
    with forced(28):
        v13 = ops.conv2d(c["x"], phase_w(c["w"]), 3, upsample=2, bias=c["bias"], group_bias=c["gb"])
    assert torch.equal(v13, c["phase"])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cin", [64, 192, 1280])
def test_the_two_phase_kernels_give_the_same_bits(dev, dtype, cin):
    c = rounding_case(dev, dtype, cin)
    wp = phase_w(c["w"])
    outs = {}
    for v in (1, 28, 0):
        with forced(v):
            outs[v] = ops.conv2d(c["x"], wp, 3, upsample=2, bias=c["bias"], group_bias=c["gb"])
    assert torch.equal(outs[1], c["phase"])
    assert torch.equal(outs[28], outs[1]), (outs[28].float() - outs[1].float()).abs().max().item()
    assert torch.equal(outs[0], outs[1])
    L.lib().omg_debug_set_glds(0)                      # the register-staged build of the 128x128 kernel
    try:
        with forced(1):
            reg = ops.conv2d(c["x"], wp, 3, upsample=2, bias=c["bias"], group_bias=c["gb"])
    finally:
        L.lib().omg_debug_set_glds(1)
    assert torch.equal(reg, outs[1])


# ------------------------------------------------------------------ slots and batches
@pytest.mark.parametrize("variant", [1, 28])
@pytest.mark.parametrize("hw", [(5, 7), (16, 16)])
def test_slot_samples_equal_the_single_slot_calls(dev, variant, hw):
    """Three samples with weight slots [0, 2, 1] in one launch == three single-sample calls with that slot's phase image, bit for bit."""
    H, W = hw
    dtype = torch.float16
    g = torch.Generator().manual_seed(H)
    x = torch.randn(3, H, W, 64, generator=g).to(dtype).to(dev)
    ws = (torch.randn(3, 320, 64, 3, 3, generator=g) * (9 * 64) ** -0.5).to(dtype).to(dev)
    bias, gb = torch.randn(320, generator=g).to(dtype).to(dev), torch.randn(3, 320, generator=g).to(dtype).to(dev)
    wp = phase_w(ws)
    assert wp.shape == (3, 4, 320, 256)
    ids = [0, 2, 1]
    with forced(variant):
        got = ops.conv2d(x, wp, 3, upsample=2, bias=bias, group_bias=gb, w_group_adapter=torch.tensor(ids, dtype=torch.int32, device=dev))
        for i, s in enumerate(ids):
            one = ops.conv2d(x[i:i + 1].contiguous(), wp[s], 3, upsample=2, bias=bias, group_bias=gb[i:i + 1].contiguous())
            assert torch.equal(got[i:i + 1], one), (i, s)
        # a sample with slot -1 is skipped: its rows keep what was there
        out = torch.full_like(got, 7.0)
        ops.conv2d(x, wp, 3, upsample=2, bias=bias, group_bias=gb, w_group_adapter=torch.tensor([1, -1, 0], dtype=torch.int32, device=dev), out=out)
    assert (out[1] == 7.0).all() and not (out[0] == 7.0).any() and not (out[2] == 7.0).any()


@pytest.mark.parametrize("hw", [(5, 7), (16, 16)])
def test_a_batch_equals_its_single_samples(dev, hw):
    """B = 4 == four B = 1 calls, bit for bit: a row's arithmetic does not depend on M, on the tile count or on the kernel the chooser takes."""
    H, W = hw
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator().manual_seed(W)
        x = torch.randn(4, H, W, 128, generator=g).to(dtype).to(dev)
        w = (torch.randn(320, 128, 3, 3, generator=g) * (9 * 128) ** -0.5).to(dtype).to(dev)
        bias, gb = torch.randn(320, generator=g).to(dtype).to(dev), torch.randn(4, 320, generator=g).to(dtype).to(dev)
        wp = phase_w(w)
        got = ops.conv2d(x, wp, 3, upsample=2, bias=bias, group_bias=gb)
        for i in range(4):
            one = ops.conv2d(x[i:i + 1].contiguous(), wp, 3, upsample=2, bias=bias, group_bias=gb[i:i + 1].contiguous())
            assert torch.equal(got[i:i + 1], one), (dtype, i)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_conv2d_module_takes_the_phase_form_with_merged_slots(dev, dtype):
    """``Conv2d.forward(upsample=True)`` with merged weight slots: the slots' phase image, a slot per sample; the sample on slot 0 is the plain
    call bit for bit; a layer that also carries un-merged LoRA factors stays on the direct form in every mode."""
    from omg_amd.modules import LoraState
    g = torch.Generator().manual_seed(11)
    m = Conv2d(64, 64, 3, dtype=dtype, device=dev)
    m.weight.data.copy_((torch.randn(64, 64, 3, 3, generator=g) * (9 * 64) ** -0.5).to(dtype))
    m.bias.data.copy_(torch.randn(64, generator=g).to(dtype))
    base = ops.pack_conv_weight(m.weight.data)
    m.w_slots = torch.stack([base, (base.float() + 0.02 * torch.randn(base.shape, generator=g).to(dev)).to(dtype)]).contiguous()
    x = torch.randn(3, 12, 10, 64, generator=g).to(dtype).to(dev)
    ids = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    m.lora_state = LoraState(ids, 3, merged=True)
    y_m = m(x, upsample=True)
    want = ops.conv2d(x, m.slot_phase_weight(), 3, upsample=2, bias=m.bias, w_group_adapter=ids)
    assert torch.equal(y_m, want)
    m.lora_state = None
    y_0 = m(x, upsample=True)
    assert torch.equal(y_0, ops.conv2d(x, m.phase_weight(), 3, upsample=2, bias=m.bias))
    assert torch.equal(y_m[1], y_0[1]) and not torch.equal(y_m[0], y_0[0])
    direct = ops.conv2d(x, m.packed_weight(), 3, upsample=True, bias=m.bias)
    assert not torch.equal(y_0, direct)
    # segment mode: the phase form takes no K-segment, so the 1x1 up conv is added onto the phase result of the samples that have an adapter
    m.lora_down = (torch.randn(2, 8, 9 * 64, generator=g) * (9 * 64) ** -0.5).to(dtype).to(dev)
    m.lora_up = (torch.randn(2, 64, 8, generator=g) * 0.1).to(dtype).to(dev)
    assert torch.equal(m(x, upsample=True), y_0)                       # LoRA stacks on the layer do not change the plain call
    sl = torch.tensor([1, -1, 0], dtype=torch.int32, device=dev)
    m.lora_state = LoraState(sl, 3, merged=False)
    y_s = m(x, upsample=True)
    assert torch.equal(y_s[1], y_0[1])                                 # the sample without adapter: the plain conv's bits
    t = ops.conv2d(x, m.lora_down, 3, upsample=True, w_group_adapter=sl)
    for i, s_ in ((0, 1), (2, 0)):
        want_i = y_0[i].double() + t[i].double() @ m.lora_up[s_].double().T
        torch.testing.assert_close(y_s[i].double(), want_i, rtol=TOL[dtype], atol=TOL[dtype])
        assert not torch.equal(y_s[i], y_0[i])
        one = LoraState(sl[i:i + 1].contiguous(), 1, merged=False)
        m.lora_state = one
        assert torch.equal(m(x[i:i + 1].contiguous(), upsample=True)[0], y_s[i])      # batched == single
    m.lora_up = torch.zeros_like(m.lora_up)                            # zero up factors: the plain conv, bit for bit
    m.lora_state = LoraState(sl, 3, merged=False)
    assert torch.equal(m(x, upsample=True), y_0)
    m.lora_state = None


# ------------------------------------------------------------------ refusals
def test_the_phase_form_refuses_what_it_does_not_compute(dev):
    dtype = torch.float16
    x = torch.zeros(1, 4, 4, 64, dtype=dtype, device=dev)
    wp = torch.zeros(4, 8, 256, dtype=dtype, device=dev)
    for kw in (dict(stride=2), dict(x2=x), dict(residual=torch.zeros(1, 8, 8, 8, dtype=dtype, device=dev)),
               dict(lora=ops.LoraSpec(torch.zeros(64, 8, dtype=dtype, device=dev), torch.zeros(8, 8, dtype=dtype, device=dev), None))):
        with pytest.raises(L.OmgHipError):
            ops.conv2d(x, wp, 3, upsample=2, **kw)
    with pytest.raises(L.OmgHipError):
        ops.conv2d(x, torch.zeros(8, 64, dtype=dtype, device=dev), 1, upsample=2)
    # the C entry point itself: an error code and no launch, not a fall-back
    y = torch.zeros(1, 8, 8, 8, dtype=dtype, device=dev)

    def args(**over):
        a = L.Conv2dArgs()
        a.dtype = L.OMG_F16
        a.B, a.Hin, a.Win, a.C1, a.C2, a.Hout, a.Wout, a.Cout = 1, 4, 4, 64, 0, 8, 8, 8
        a.ksize, a.stride, a.upsample = 3, 1, 2
        a.X1, a.W, a.Y, a.out_scale = x.data_ptr(), wp.data_ptr(), y.data_ptr(), 1.0
        for k, v in over.items():
            setattr(a, k, v)
        return a
    stream = torch.cuda.current_stream().cuda_stream
    assert L.lib().omg_conv2d(C.byref(args()), stream) == 0
    assert L.lib().omg_conv2d(C.byref(args(ksize=1)), stream) != 0
    assert L.lib().omg_conv2d(C.byref(args(stride=2, Hout=4, Wout=4)), stream) != 0
    assert L.lib().omg_conv2d(C.byref(args(X2=x.data_ptr(), C2=64)), stream) != 0
    assert L.lib().omg_conv2d(C.byref(args(upsample=3)), stream) != 0
    sa = L.Conv2dSlotsArgs()
    C.memmove(C.byref(sa.conv), C.byref(args()), C.sizeof(L.Conv2dArgs))
    sa.K2, sa.A2, sa.W2, sa.lda2, sa.ldw2 = 8, x.data_ptr(), wp.data_ptr(), 8, 8
    assert L.lib().omg_conv2d_slots(C.byref(sa), stream) != 0            # the LoRA K-segment
    sa.K2 = 0
    assert L.lib().omg_conv2d_slots(C.byref(sa), stream) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ module level
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_unet_forward_takes_the_phase_form(dev, dtype):
    """The tiny UNet's two upsample convolutions run the phase form; with the direct form forced through ``Conv2d.phase_upsample`` the forward
    differs (other roundings) by no more than the module tolerance of tests/test_unet_gpu.py."""
    from oracle import unet as ou
    from omg_amd.unet import UNet2DConditionModel, UNetConfig
    cfg, ocfg = UNetConfig.tiny(), ou.UNetConfig.tiny()
    sd = ou.init_state_dict(ocfg, seed=0, dtype=dtype)
    unet = UNet2DConditionModel(cfg, dtype=dtype, device=dev)
    unet.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    g = torch.Generator().manual_seed(0)
    n = cfg.sample_size
    x = torch.randn(2, 4, n, n, generator=g).to(dev)
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).to(dtype).to(dev)
    te = torch.randn(2, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g).to(dtype).to(dev)
    tid = torch.tensor([[n * 8.0, n * 8.0, 0, 0, n * 8.0, n * 8.0]] * 2).to(dev)

    def run():
        return unet(x, 981, encoder_hidden_states=ctx, added_cond_kwargs={"text_embeds": te, "time_ids": tid}, return_dict=False)[0].float().cpu()
    ups = [m for m in unet.modules() if isinstance(m, Conv2d) and m.upsamples]
    assert len(ups) == 2 and all(m._phase_form(True, None, None) for m in ups)
    phase = run()
    assert all("wp" in m._packed for m in ups)                     # the phase image was built and used
    assert torch.equal(run(), phase)
    assert Conv2d.phase_upsample is True
    Conv2d.phase_upsample = False
    try:
        direct = run()
    finally:
        Conv2d.phase_upsample = True
    d = (phase - direct).abs().max().item()
    print(f"tiny UNet {dtype}: phase vs direct max|d|={d:.3e}, rms {direct.pow(2).mean().sqrt().item():.3f}")
    assert not torch.equal(phase, direct)
    assert d <= TOL_UNET[dtype]
