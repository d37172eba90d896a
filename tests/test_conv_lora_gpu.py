"""LoRA on convolution layers (-m gpu): omg_conv2d_slots (a weight slot per sample, the LoRA second K-segment), the Conv2d module's
merged / segment forward, and a UNet whose adapters target Linear AND conv layers, against the float64 helper of
tests/_conv_lora_oracle.py and oracle/unet.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from omg_amd.lora import LoraAdapter, LoraBank
from omg_amd.modules import Conv2d, LoraState
from omg_amd.unet import UNet2DConditionModel, UNetConfig
from oracle import unet as ou
from tests import _conv_lora_oracle as co

DTYPES = [torch.float16, torch.bfloat16]
# DESIGN §3 tolerance table, kernel level
TOL = {torch.float16: dict(rtol=2e-3, atol=2e-3), torch.bfloat16: dict(rtol=1.6e-2, atol=1.6e-2)}
VARIANTS = [1, 13, 14, 15, 24, 25, 28]


def rnd(*shape, dtype, dev, scale=1.0, seed=None):
    g = torch.Generator().manual_seed(seed if seed is not None else sum(shape) + 17)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def close(out, ref, dtype, factor=1.0):
    t = TOL[dtype]
    torch.testing.assert_close(out.double().cpu(), ref.double(), rtol=t["rtol"] * factor, atol=t["atol"] * factor)


# (name, Hin, Win, C1, C2, Cout, ksize, stride, upsample, epilogue flags)
FORMS = [
    ("12x10 per-row group bias", 12, 10, 64, 0, 64, 3, 1, False, dict(bias=1, gb=1)),                  # 120 rows: less than one tile
    ("20x12 concat residual", 20, 12, 64, 64, 192, 3, 1, False, dict(bias=1, res=1, out_scale=0.5)),   # 240 rows: a 128 tile + a partial one
    ("16x16 folded group bias silu", 16, 16, 64, 0, 320, 3, 1, False, dict(gb=1, silu=1)),             # 256 rows: the bias is folded
    ("stride 2", 24, 20, 64, 0, 64, 3, 2, False, dict(bias=1)),                                        # -> 12 x 10
    ("upsample", 10, 6, 64, 0, 192, 3, 1, True, dict(res=1)),                                          # -> 20 x 12
    ("1x1 concat", 20, 12, 64, 64, 320, 1, 1, False, dict(bias=1, gb=1)),
    ("24x20 all", 24, 20, 64, 0, 320, 3, 1, False, dict(bias=1, gb=1, res=1, out_scale=0.5, silu=1)),  # 480 rows: a 256 tile + a partial one
]


def make_case(form, B, n_slots, dtype, dev, seed=0):
    _, Hin, Win, C1, C2, Cout, k, stride, ups, fl = form
    K = k * k * (C1 + C2)
    Hl, Wl = (2 * Hin, 2 * Win) if ups else (Hin, Win)
    pad = 1 if k == 3 else 0
    Ho, Wo = (Hl + 2 * pad - k) // stride + 1, (Wl + 2 * pad - k) // stride + 1
    c = dict(k=k, stride=stride, ups=ups, Ho=Ho, Wo=Wo, Cout=Cout, K=K)
    c["x1"] = rnd(B, Hin, Win, C1, dtype=dtype, dev=dev, seed=seed + 1)
    c["x2"] = rnd(B, Hin, Win, C2, dtype=dtype, dev=dev, seed=seed + 2) if C2 else None
    c["w"] = rnd(n_slots, Cout, K, dtype=dtype, dev=dev, scale=K ** -0.5, seed=seed + 3)
    c["bias"] = rnd(Cout, dtype=dtype, dev=dev, seed=seed + 4) if fl.get("bias") else None
    c["gb"] = rnd(B, Cout, dtype=dtype, dev=dev, seed=seed + 5) if fl.get("gb") else None
    c["res"] = rnd(B, Ho, Wo, Cout, dtype=dtype, dev=dev, seed=seed + 6) if fl.get("res") else None
    c["out_scale"] = fl.get("out_scale", 1.0)
    c["act"] = L.ACT_SILU if fl.get("silu") else L.ACT_NONE
    return c


def run_conv(c, w, rows=None, **kw):
    """ops.conv2d of the case on the samples ``rows`` (a slice) with weight ``w``."""
    s = rows if rows is not None else slice(None)
    sl = lambda t: None if t is None else t[s].contiguous()
    return ops.conv2d(sl(c["x1"]), w, c["k"], stride=c["stride"], upsample=c["ups"], x2=sl(c["x2"]), bias=c["bias"], group_bias=sl(c["gb"]),
                      residual=sl(c["res"]), out_scale=c["out_scale"], act=c["act"], **kw)


# ------------------------------------------------------------------ slots, bitwise
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_slot_conv_is_bitwise_the_single_sample_convs(dev, dtype, variant):
    """w [3, Cout, K] with slots [2, 0, 1] on B = 3 equals three single-sample ops.conv2d calls with the respective weight, under every
    tile variant the chooser can return; and with all slots equal and the weight repeated it equals the plain batch conv."""
    lib = L.lib()
    ids = torch.tensor([2, 0, 1], dtype=torch.int32, device=dev)
    same = torch.tensor([1, 1, 1], dtype=torch.int32, device=dev)
    try:
        lib.omg_debug_set_gemm_variant(variant)
        for form in FORMS:
            c = make_case(form, 3, 3, dtype, dev)
            got = run_conv(c, c["w"], w_group_adapter=ids)
            for b, s in enumerate([2, 0, 1]):
                want = run_conv(c, c["w"][s].contiguous(), rows=slice(b, b + 1))
                assert torch.equal(got[b:b + 1], want), f"{form[0]} sample {b}: max diff {(got[b:b + 1].float() - want.float()).abs().max().item()}"
            rep = c["w"][1:2].repeat(3, 1, 1).contiguous()
            assert torch.equal(run_conv(c, rep, w_group_adapter=same), run_conv(c, c["w"][1].contiguous())), form[0]
    finally:
        lib.omg_debug_set_gemm_variant(0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_heuristic_variant_slot_conv_is_bitwise_too(dev, dtype):
    lib = L.lib()
    lib.omg_debug_set_gemm_variant(0)
    ids = torch.tensor([2, 0, 1], dtype=torch.int32, device=dev)
    for form in FORMS:
        c = make_case(form, 3, 3, dtype, dev)
        got = run_conv(c, c["w"], w_group_adapter=ids)
        for b, s in enumerate([2, 0, 1]):
            assert torch.equal(got[b:b + 1], run_conv(c, c["w"][s].contiguous(), rows=slice(b, b + 1))), (form[0], b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_persistent_walk_steps_between_samples_of_different_slots(dev, dtype):
    """Variant 25 with the grid capped at eight blocks: B = 6 samples of 480 rows x 320 columns = 24 tiles with alternating slots, so that one
    block walks tiles of different weights (the next tile's weight descriptor is set while the current tile's last stage runs)."""
    lib = L.lib()
    slots = [1, 0, 1, 0, 1, 0]
    ids = torch.tensor(slots, dtype=torch.int32, device=dev)
    try:
        for form in (FORMS[6], FORMS[2], FORMS[1]):          # persistent generic form (4), folded bias + SiLU (4), residual (2: one tile per block)
            c = make_case(form, 6, 2, dtype, dev)
            lib.omg_debug_set_gemm_variant(1)
            want = torch.cat([run_conv(c, c["w"][s].contiguous(), rows=slice(b, b + 1)) for b, s in enumerate(slots)])
            for cap in (0x10000, 0):
                lib.omg_debug_set_gemm_variant(25 | (cap << 8))
                got = run_conv(c, c["w"], w_group_adapter=ids)
                assert torch.equal(got, want), f"{form[0]} cap {cap:#x}: max diff {(got.float() - want.float()).abs().max().item()}"
    finally:
        lib.omg_debug_set_gemm_variant(0)


# ------------------------------------------------------------------ the second K-segment
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K2", [8, 16, 72])
def test_segment_adds_the_lora_product_into_the_accumulator(dev, dtype, K2):
    """K2 = 8 (less than one K stage), 16, 72 (more than one stage): base conv + A2 . W2[slot]^T on the same 16-bit operands in float64;
    a slot -1 sample is bitwise the plain conv of that sample."""
    slots = [1, -1, 0]
    ids = torch.tensor(slots, dtype=torch.int32, device=dev)
    for glds in (1, 0):
        L.lib().omg_debug_set_glds(glds)
        try:
            for form in FORMS:
                c = make_case(form, 3, 1, dtype, dev)
                w = c["w"][0].contiguous()
                a2 = rnd(3 * c["Ho"] * c["Wo"], K2, dtype=dtype, dev=dev, seed=11)
                w2 = rnd(2, c["Cout"], K2, dtype=dtype, dev=dev, scale=0.1, seed=12)
                got = run_conv(c, w, lora=ops.LoraSpec(a2, w2, ids))
                plain = run_conv(c, w)
                assert torch.equal(got[1], plain[1]), form[0]
                cpu = lambda t: None if t is None else t.cpu()
                w_oihw = w.cpu().double().view(c["Cout"], c["k"], c["k"], -1).permute(0, 3, 1, 2)
                extra = torch.zeros(3, c["Ho"], c["Wo"], c["Cout"], dtype=torch.float64)
                for b, s in enumerate(slots):
                    if s >= 0:
                        rows = a2.cpu().double().view(3, c["Ho"] * c["Wo"], K2)[b]
                        extra[b] = (rows @ w2[s].cpu().double().T).view(c["Ho"], c["Wo"], c["Cout"])
                ref = co.conv_nhwc(c["x1"].cpu(), w_oihw, x2=cpu(c["x2"]), stride=c["stride"], upsample=c["ups"], bias=cpu(c["bias"]),
                                   group_bias=cpu(c["gb"]), residual=cpu(c["res"]), out_scale=c["out_scale"], silu=c["act"] == L.ACT_SILU, extra=extra)
                close(got, ref, dtype)
        finally:
            L.lib().omg_debug_set_glds(1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_down_conv_skips_samples_without_adapter(dev, dtype):
    """The LoRA-down launch (weight slots, slot -1 skipped): the skipped sample's rows keep the canary, the others are the plain conv."""
    ids = torch.tensor([1, -1, 0], dtype=torch.int32, device=dev)
    for form in FORMS:
        c = make_case(form, 3, 2, dtype, dev)
        c = dict(c, bias=None, gb=None, res=None, out_scale=1.0, act=L.ACT_NONE)
        wd = rnd(2, 16, c["K"], dtype=dtype, dev=dev, scale=c["K"] ** -0.5, seed=21)
        out = torch.full((3, c["Ho"], c["Wo"], 16), 7.0, dtype=dtype, device=dev)
        run_conv(c, wd, w_group_adapter=ids, out=out)
        assert bool((out[1] == 7.0).all()), form[0]
        for b, s in ((0, 1), (2, 0)):
            assert torch.equal(out[b:b + 1], run_conv(c, wd[s].contiguous(), rows=slice(b, b + 1))), (form[0], b)


# ------------------------------------------------------------------ validation
def test_every_requirement_of_the_new_entry_point_is_refused_without_a_launch(dev):
    dtype = torch.float16
    lib = L.lib()
    B, H, W, Cin, Cout, K2 = 2, 8, 8, 64, 64, 16
    x = rnd(B, H, W, Cin, dtype=dtype, dev=dev)
    w = rnd(2, Cout, 9 * Cin, dtype=dtype, dev=dev, scale=0.05)
    a2 = rnd(B * H * W, K2, dtype=dtype, dev=dev)
    w2 = rnd(2, Cout, K2, dtype=dtype, dev=dev)
    ids = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    y = torch.full((B, H, W, Cout), 7.0, dtype=dtype, device=dev)

    def args():
        a = L.Conv2dSlotsArgs()
        cv = a.conv
        cv.dtype, cv.B, cv.Hin, cv.Win, cv.C1, cv.C2, cv.Hout, cv.Wout, cv.Cout = L.OMG_F16, B, H, W, Cin, 0, H, W, Cout
        cv.ksize, cv.stride, cv.upsample, cv.out_scale = 3, 1, 0, 1.0
        cv.X1, cv.W, cv.Y = x.data_ptr(), w.data_ptr(), y.data_ptr()
        a.group_adapter, a.w_slot_stride = ids.data_ptr(), w.stride(0)
        a.A2, a.lda2, a.W2, a.ldw2, a.w2_slot_stride, a.K2 = a2.data_ptr(), K2, w2.data_ptr(), K2, w2.stride(0), K2
        return a

    good = args()
    assert lib.omg_conv2d_slots(C.byref(good), None) == 0
    torch.cuda.synchronize()
    assert not bool((y == 7.0).all())
    y.fill_(7.0)

    def bad(**kw):
        a = args()
        for k, v in kw.items():
            obj, name = (a.conv, k[5:]) if k.startswith("conv_") else (a, k)
            setattr(obj, name, v)
        return a

    cases = {
        "K2 % 8": bad(K2=12), "K2 < 0": bad(K2=-8), "w_slot_stride < 0": bad(w_slot_stride=-8), "w_slot_stride % 8": bad(w_slot_stride=Cout * 9 * Cin + 4),
        "w_slot_stride < one weight": bad(w_slot_stride=Cout * 9 * Cin - 8), "A2 null": bad(A2=None), "W2 null": bad(W2=None),
        "lda2 % 8": bad(lda2=K2 + 4), "lda2 < K2": bad(lda2=K2 - 8), "ldw2 % 8": bad(ldw2=K2 + 4), "ldw2 < K2": bad(ldw2=K2 - 8),
        "w2_slot_stride < 0": bad(w2_slot_stride=-8), "w2_slot_stride % 8": bad(w2_slot_stride=Cout * K2 + 4),
        # the embedded omg_conv2d_args keep omg_conv2d's requirements
        "dtype": bad(conv_dtype=L.OMG_F32), "ksize": bad(conv_ksize=2), "stride": bad(conv_stride=3), "channels": bad(conv_C1=48), "Cout": bad(conv_Cout=60),
        "null X1": bad(conv_X1=None), "upsample with stride": bad(conv_upsample=1, conv_stride=2), "output size": bad(conv_Hout=H + 1),
        "act": bad(conv_act=L.ACT_GEGLU), "ldgb": bad(conv_group_bias=x.data_ptr(), conv_ldgb=Cout + 4),
    }
    assert lib.omg_conv2d_slots(None, None) != 0 and lib.omg_last_error()
    for name, a in cases.items():
        rc = lib.omg_conv2d_slots(C.byref(a), None)
        assert rc != 0 and lib.omg_last_error(), name
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "a refused call wrote to the output"


# ------------------------------------------------------------------ the Conv2d module
# the five layer forms of the UNet: resnet conv1 (concat input, per-sample bias), conv2 (residual), the 1x1 shortcut on the concat, the
# stride-2 downsampler, the upsampler
LAYERS = [
    ("conv1", 128, 64, 3, 1, dict(concat=True, gb=True)), ("conv2", 64, 64, 3, 1, dict(res=True)), ("conv_shortcut", 128, 192, 1, 1, dict(concat=True)),
    ("downsampler", 64, 64, 3, 2, dict()), ("upsampler", 64, 64, 3, 1, dict(ups=True)),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", LAYERS, ids=[l[0] for l in LAYERS])
def test_conv2d_module_merged_and_segment_match_the_float64_helper(dev, dtype, layer):
    _, cin, cout, k, stride, fl = layer
    B, H, W, S, r = 3, 12, 10, 2, 8
    m = Conv2d(cin, cout, k, stride=stride, dtype=dtype, device=dev)
    m.weight.data.copy_(rnd(cout, cin, k, k, dtype=dtype, dev=dev, scale=(cin * k * k) ** -0.5, seed=1))
    m.bias.data.copy_(rnd(cout, dtype=dtype, dev=dev, seed=2))
    A = [rnd(r, cin, k, k, dtype=dtype, dev=dev, scale=(cin * k * k) ** -0.5, seed=10 + s) for s in range(S)]
    Bm = [rnd(cout, r, dtype=dtype, dev=dev, scale=0.1, seed=20 + s) for s in range(S)]
    scale = 0.8
    down = torch.stack([ops.pack_conv_weight(a) for a in A]).contiguous()
    up32 = torch.stack([b.float() * scale for b in Bm])
    m.lora_down, m.lora_up = down, up32.to(dtype).contiguous()
    base = ops.pack_conv_weight(m.weight.data).float()
    m.w_slots = torch.stack([base] + [base + up32[s] @ down[s].float() for s in range(S)]).to(dtype).contiguous()
    if fl.get("concat"):
        x1, x2 = rnd(B, H, W, cin // 2, dtype=dtype, dev=dev, seed=3), rnd(B, H, W, cin // 2, dtype=dtype, dev=dev, seed=4)
    else:
        x1, x2 = rnd(B, H, W, cin, dtype=dtype, dev=dev, seed=3), None
    ups = bool(fl.get("ups"))
    Ho, Wo = (2 * H, 2 * W) if ups else ((H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1)
    gb = rnd(B, cout, dtype=dtype, dev=dev, seed=5) if fl.get("gb") else None
    res = rnd(B, Ho, Wo, cout, dtype=dtype, dev=dev, seed=6) if fl.get("res") else None
    slots = [1, -1, 0]                                   # LoRA slot per sample (-1: base weights)
    cpu = lambda t: None if t is None else t.cpu()
    ref = torch.empty(B, Ho, Wo, cout, dtype=torch.float64)
    for b, s in enumerate(slots):
        sl = lambda t: None if t is None else t[b:b + 1].cpu()
        extra = scale * co.lora_nhwc(sl(x1), A[s].cpu(), Bm[s].cpu(), x2=sl(x2), stride=stride, upsample=ups) if s >= 0 else None
        ref[b:b + 1] = co.conv_nhwc(sl(x1), m.weight.data.cpu(), x2=sl(x2), stride=stride, upsample=ups, bias=cpu(m.bias.data), group_bias=sl(gb),
                                    residual=sl(res), extra=extra)
    m.lora_state = LoraState(torch.tensor([s + 1 for s in slots], dtype=torch.int32, device=dev), B, merged=True)
    y_m = m(x1, x2=x2, upsample=ups, group_bias=gb, residual=res)
    m.lora_state = LoraState(torch.tensor(slots, dtype=torch.int32, device=dev), B, merged=False)
    y_s = m(x1, x2=x2, upsample=ups, group_bias=gb, residual=res)
    m.lora_state = None
    y_0 = m(x1, x2=x2, upsample=ups, group_bias=gb, residual=res)
    assert torch.equal(y_m[1], y_0[1]) and torch.equal(y_s[1], y_0[1])          # the sample without adapter is the plain conv
    assert not torch.equal(y_m[0], y_0[0])
    close(y_m, ref, dtype)
    close(y_s, ref, dtype)
    close(y_m, y_s.double().cpu(), dtype, factor=2.0)


# ------------------------------------------------------------------ UNet
UNET_TOL = {torch.float16: 3e-2, torch.bfloat16: 2e-1}      # the module tolerance of tests/test_unet_gpu.py


conv_targets, make_conv_lora = co.conv_targets, co.make_conv_lora


@pytest.fixture(scope="module")
def unet_case(dev):
    out = {}

    def get(dtype):
        if dtype not in out:
            cfg, ocfg = UNetConfig.tiny(), ou.UNetConfig.tiny()
            sd = ou.init_state_dict(ocfg, seed=0, dtype=dtype)
            unet = UNet2DConditionModel(cfg, dtype=dtype, device=dev)
            unet.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
            scale = 0.8
            lin, conv, fns = {}, {}, {}
            for n, seed in (("a", 100), ("b", 101)):
                lin[n], fns[n] = ou.make_lora(ocfg, ou.lora_target_names(ocfg), 8, seed, scale, dtype)
                conv[n] = make_conv_lora(ocfg, conv_targets(ocfg), 8, seed + 50, dtype)
            adapters = [LoraAdapter(n, {k: (a.to(dev), b.to(dev)) for k, (a, b) in {**lin[n], **conv[n]}.items()}) for n in ("a", "b")]
            bank = LoraBank(unet, adapters)
            g = torch.Generator().manual_seed(3)
            L_ = cfg.sample_size
            x = torch.randn(4, 4, L_, L_, generator=g)
            ctx = torch.randn(4, 77, cfg.cross_attention_dim, generator=g).to(dtype).float()
            te = torch.randn(4, 64, generator=g).to(dtype).float()
            tid = torch.tensor([[L_ * 8.0, L_ * 8.0, 0, 0, L_ * 8.0, L_ * 8.0]] * 4)
            refs = []
            for b, n in enumerate([None, "a", "b", "a"]):
                sdn = sd if n is None else co.merged_state_dict(sd, conv[n], scale)
                refs.append(ou.unet_forward(sdn, ocfg, x[b:b + 1], 981, ctx[b:b + 1], te[b:b + 1], tid[b:b + 1], lora=None if n is None else fns[n]))
            out[dtype] = dict(unet=unet, bank=bank, x=x, ctx=ctx, te=te, tid=tid, ref=torch.cat(refs), scale=scale)
        return out[dtype]

    return get


def run_unet(c, dev, dtype, rows=slice(None), state=None):
    unet = c["unet"]
    unet.set_lora_state(state)
    try:
        return unet(c["x"][rows].to(dev), 981, encoder_hidden_states=c["ctx"][rows].to(dev).to(dtype),
                    added_cond_kwargs={"text_embeds": c["te"][rows].to(dev).to(dtype), "time_ids": c["tid"][rows].to(dev)})[0].float().cpu()
    finally:
        unet.set_lora_state(None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["merged", "segment"])
def test_unet_with_linear_and_conv_adapters_per_sample(dev, dtype, mode, unet_case):
    """Tiny SDXL topology, B = 4, slots [base, a, b, a], adapters on Linear and conv targets, against oracle/unet.py run per sample on a state
    dict whose conv weights are merged in fp32 by the helper plus the lora= callback for the Linear half; batched == single, bitwise."""
    c = unet_case(dtype)
    c["bank"].build([(("a", 1.0),), (("b", 1.0),)], scale=c["scale"], mode=mode)
    off = 1 if mode == "merged" else 0
    slots = [-1 + off, 0 + off, 1 + off, 0 + off]
    mk = lambda s: LoraState(torch.tensor(s, dtype=torch.int32, device=dev), len(s), merged=mode == "merged")
    got = run_unet(c, dev, dtype, state=mk(slots))
    err = (got - c["ref"]).abs().max().item()
    print(f"unet conv lora {mode} {dtype}: max|d| = {err:.3e}")
    assert err < UNET_TOL[dtype]
    plain = run_unet(c, dev, dtype)
    assert torch.equal(got[0], plain[0]) and (got[1] - plain[1]).abs().max() > 1e-3
    for b in range(4):
        one = run_unet(c, dev, dtype, rows=slice(b, b + 1), state=mk(slots[b:b + 1]))
        assert torch.equal(one[0], got[b]), f"sample {b}"
    c["bank"].clear()


def test_unet_conv_slots_in_mx8_mode_run_the_16_bit_kernel(dev, unet_case):
    """--dtype fp8: a conv that carries LoRA slots has mx8_ok() False, so it runs the 16-bit slot kernel (and its GroupNorm writes a 16-bit
    map); the forward stays within the MX module bound of tests/test_mx8_gpu.py."""
    from omg_amd.unet import ResnetBlock2D
    dtype = torch.float16
    c = unet_case(dtype)
    unet = c["unet"]
    c["bank"].build([(("a", 1.0),), (("b", 1.0),)], scale=c["scale"], mode="merged")
    unet.set_conv_precision("mx8")
    try:
        res = [m for m in unet.modules() if isinstance(m, ResnetBlock2D)]
        assert all(m.conv1.mx8 and not m.conv1.mx8_ok() and not m.conv2.mx8_ok() for m in res)      # those layers run in 16 bits
        got = run_unet(c, dev, dtype, state=LoraState(torch.tensor([0, 1, 2, 1], dtype=torch.int32, device=dev), 4, merged=True))
        rms = c["ref"].pow(2).mean().sqrt().item()
        e_max, e_rms = (got - c["ref"]).abs().max().item() / rms, (got - c["ref"]).pow(2).mean().sqrt().item() / rms
        print(f"conv slots in mx8 conv mode: max|d| / rms {e_max:.2e}, rms error {e_rms:.2e}")
        assert e_max < 0.7 and e_rms < 0.16      # the MX-fp8 Linear + conv bound of tests/test_mx8_gpu.py
    finally:
        unet.set_conv_precision("fp16")
        c["bank"].clear()
