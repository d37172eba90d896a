"""The phase form of the nearest-2x upsample + 3x3 convolution (DESIGN §5 "The upsample convolution: four 2x2 phases"), host side: the
weight image ``ops.pack_conv_weight_phase`` against the float64 identity, its caches on ``Conv2d``, and the code objects of the phase kernels."""
import os

import pytest
import torch
import torch.nn.functional as F

from omg_amd import modules, ops
from omg_amd.modules import Conv2d
from tests import _codeobj

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omg_amd", "csrc", "libomg_hip.so")


def phase_conv_reference(x_nchw: torch.Tensor, wp: torch.Tensor) -> torch.Tensor:
    """The four 2x2 convolutions exactly as the kernels run them, in torch: phase 2 py + px, tap (a, c) reads source pixel
    (y - 1 + py + a, x - 1 + px + c), zeros outside; its result is output pixel (2 y + py, 2 x + px).  ``wp``: [4, Cout, 4 * Cin]."""
    B, Cin, H, W = x_nchw.shape
    Cout = wp.shape[1]
    y = x_nchw.new_zeros((B, Cout, 2 * H, 2 * W))
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        k = wp[ph].view(Cout, 2, 2, Cin).permute(0, 3, 1, 2)
        y[:, :, py::2, px::2] = F.conv2d(F.pad(x_nchw, (1 - px, px, 1 - py, py)), k)
    return y


@pytest.mark.parametrize("H", [1, 4, 5, 6, 7])
@pytest.mark.parametrize("W", [1, 4, 5, 6, 7])
def test_phase_image_is_the_upsampled_convolution_in_float64(H, W):
    g = torch.Generator().manual_seed(H * 8 + W)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(5, 3, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    wp = ops.pack_conv_weight_phase(w)
    assert wp.shape == (4, 5, 12) and wp.dtype == torch.float64 and wp.is_contiguous()
    assert (phase_conv_reference(x, wp) - want).abs().max().item() <= 1e-12


def test_phase_image_sums_in_fp32_and_rounds_once():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(8, 64, 3, 3, generator=g).to(torch.float16)
    wp = ops.pack_conv_weight_phase(w)
    assert wp.dtype == torch.float16 and wp.shape == (4, 8, 256)
    exact = ops.pack_conv_weight_phase(w.double())           # sums of at most four fp16 values: exact in float64
    assert torch.equal(wp, exact.to(torch.float16))         # one rounding of the exact sum
    # phase 0, tap (1, 1) is the sum of the four taps (1..2, 1..2); phase 3, tap (0, 0) of the four taps (0..1, 0..1)
    assert torch.equal(wp[0].view(8, 4, 64)[:, 3], w[:, :, 1:, 1:].double().sum((2, 3)).to(torch.float16))
    assert torch.equal(wp[3].view(8, 4, 64)[:, 0], w[:, :, :2, :2].double().sum((2, 3)).to(torch.float16))
    assert torch.equal(wp[1].view(8, 4, 64)[:, 1], w[:, :, 0, 2])      # phase (0, 1), tap (0, 1): the single tap (0, 2)


def test_phase_image_keeps_a_leading_slot_dimension():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(3, 8, 64, 3, 3, generator=g).to(torch.bfloat16)
    wp = ops.pack_conv_weight_phase(w)
    assert wp.shape == (3, 4, 8, 256) and wp.is_contiguous()
    for s in range(3):
        assert torch.equal(wp[s], ops.pack_conv_weight_phase(w[s]))


def _conv(seed=0, cin=64, cout=8):
    c = Conv2d(cin, cout, 3, dtype=torch.float16)
    g = torch.Generator().manual_seed(seed)
    c.load_state_dict({"weight": torch.randn(cout, cin, 3, 3, generator=g).to(torch.float16), "bias": torch.zeros(cout, dtype=torch.float16)})
    return c


def test_phase_weight_is_cached_and_dropped_with_the_packed_weight():
    c = _conv(0)
    wp = c.phase_weight()
    assert c.phase_weight() is wp and torch.equal(wp, ops.pack_conv_weight_phase(c.weight.data))
    epoch = modules.pointer_epoch()
    g = torch.Generator().manual_seed(9)
    c.load_state_dict({"weight": torch.randn(8, 64, 3, 3, generator=g).to(torch.float16), "bias": torch.zeros(8, dtype=torch.float16)})
    assert modules.pointer_epoch() > epoch                  # graphs that hold the old image's pointer are dropped
    wp2 = c.phase_weight()
    assert wp2 is not wp and torch.equal(wp2, ops.pack_conv_weight_phase(c.weight.data)) and not torch.equal(wp2, wp)
    c.invalidate_packed()
    assert c.phase_weight() is not wp2


def test_slot_phase_image_follows_the_slots():
    c = _conv(1)
    base = ops.pack_conv_weight(c.weight.data)
    g = torch.Generator().manual_seed(5)
    c.w_slots = torch.stack([base, (base.float() + 0.01 * torch.randn(base.shape, generator=g)).to(base.dtype)]).contiguous()
    sp = c.slot_phase_weight()
    assert sp.shape == (2, 4, 8, 256) and c.slot_phase_weight() is sp
    assert torch.equal(sp[0], c.phase_weight())              # slot 0 is the base weight: the same image, bit for bit
    oihw1 = c.w_slots[1].view(8, 3, 3, 64).permute(0, 3, 1, 2)
    assert torch.equal(sp[1], ops.pack_conv_weight_phase(oihw1))
    epoch = modules.pointer_epoch()
    c.w_slots = c.w_slots.flip(0).contiguous()              # replaced slots: a new image, and the pointer epoch moves
    sp2 = c.slot_phase_weight()
    assert sp2 is not sp and torch.equal(sp2[1], sp[0]) and torch.equal(sp2[0], sp[1])
    assert modules.pointer_epoch() > epoch
    epoch = modules.pointer_epoch()
    c.drop_slot_phase()
    assert c._slot_phase is None and modules.pointer_epoch() > epoch


def test_the_phase_form_is_chosen_by_the_layer_alone():
    c = _conv(2)
    x2 = torch.zeros(1)
    assert c._phase_form(True, None, None)
    assert not c._phase_form(False, None, None)
    assert not c._phase_form(True, x2, None) and not c._phase_form(True, None, x2)
    c.phase_upsample = False                                # the attribute that forces the direct form
    assert not c._phase_form(True, None, None)
    c.phase_upsample = True
    c.lora_down = torch.zeros(1, 8, 9 * 64, dtype=torch.float16)      # LoRA stacks on the layer do not change the form
    assert c._phase_form(True, None, None)
    c.lora_down = None
    assert Conv2d.phase_upsample is True
    assert not Conv2d(64, 8, 1, dtype=torch.float16)._phase_form(True, None, None)
    assert not Conv2d(64, 8, 3, stride=2, dtype=torch.float16)._phase_form(True, None, None)


@pytest.mark.skipif(not _codeobj.available(LIB), reason="libomg_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_the_phase_kernels_use_no_scratch():
    """gemm_phase_kernel (128x128: fp16 / bf16 x LDS-DMA / register staged) and gemm_phase_kernel_v13 (256x320: fp16 / bf16 x bias-only / generic
    epilogue): kernels of their own, so that no other instantiation changes; no scratch, no spills, the 128x128 one still two blocks per CU, the
    256x320 one with its 256 accumulators in AGPRs."""
    ks = _codeobj.kernels(LIB)
    v1 = {n: k for n, k in ks.items() if "17gemm_phase_kernelI" in n}
    v13 = {n: k for n, k in ks.items() if "21gemm_phase_kernel_v13I" in n}
    assert len(v1) == 4 and len(v13) == 4, (sorted(v1), sorted(v13))
    for n, k in {**v1, **v13}.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256, n
    for n, k in v1.items():
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, (n, k)
    for n, k in v13.items():
        assert k["agpr_count"] == 256 and k["group_segment_fixed_size"] == 0, (n, k)
