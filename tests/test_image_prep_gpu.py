"""ops.image_prep on the GPU (-m gpu): Pillow's resize on the device, bit for bit, and the device branches of the preprocessors.

Every comparison is ``torch.equal``.  The expected images are the installed Pillow's outputs stored in tests/golden/image_prep.npz
(make_golden_image_prep.py); an image the fixture does not hold goes through image_prep.resize_reference, which tests/test_image_prep.py
holds against the fixture and against Pillow.  The planar output is compared with the host expression written out here: the lookup of
the resized image, the zero pad at the right and bottom, the cast."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import dpt as hip_dpt
from omg_amd import grounded_sam as gs
from omg_amd import image_prep as ip
from omg_amd import ops, sam as hip_sam, segment_anything as sa
from tests import sam_torch, sam_vit_torch as vt
from tests.test_image_prep import CASES, RESAMPLE, name

HERE = os.path.dirname(os.path.abspath(__file__))
CANARY = 1232.0                # exact in bfloat16


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(HERE, "golden", "image_prep.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("resample", RESAMPLE)
@pytest.mark.parametrize("case", CASES, ids=name)
def test_uint8_output_equals_pillow(dev, gold, case, resample):
    """Batch 1 (a [H, W, 3] tensor) and batch 2 (the image and its complement, the second expected from the numpy model)."""
    a = gold["in." + name(case)]
    want = torch.from_numpy(gold[f"out.{name(case)}.{resample}"])
    oh, ow = case[2], case[3]
    got = ops.image_prep(torch.from_numpy(a).to(dev), (oh, ow), resample)
    assert got.dtype == torch.uint8 and got.shape == (oh, ow, 3) and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    two = np.stack([a, 255 - a])
    got2 = ops.image_prep(torch.from_numpy(two).to(dev), (oh, ow), resample)
    assert got2.shape == (2, oh, ow, 3)
    assert torch.equal(got2[0].cpu(), want)
    assert torch.equal(got2[1].cpu(), torch.from_numpy(ip.resize_reference(two[1], (ow, oh), resample)))


def test_an_image_that_is_not_dword_aligned(dev, gold):
    """The second image of a batch of 37 x 53 x 3 = 5883 bytes starts at an odd address: the horizontal pass reads it from global memory."""
    case = CASES[0]
    a = gold["in." + name(case)]
    both = torch.from_numpy(np.stack([a, a])).to(dev)
    assert both[1].data_ptr() % 4 != 0 and both[1].is_contiguous()
    for r in RESAMPLE:
        assert torch.equal(ops.image_prep(both[1], (case[2], case[3]), r).cpu(), torch.from_numpy(gold[f"out.{name(case)}.{r}"]))


def host_planar(resized: np.ndarray, lut: torch.Tensor, pad_hw, dtype) -> torch.Tensor:
    """lookup -> pad -> cast of one resized HWC image on the host; ``lut`` fp32 [3, 256]."""
    idx = torch.from_numpy(resized.astype(np.int64))
    x = torch.stack([lut[c][idx[..., c]] for c in range(3)])
    x = torch.nn.functional.pad(x, (0, pad_hw[1] - x.shape[2], 0, pad_hw[0] - x.shape[1]))
    return x.to(dtype)


def luts32(dev):
    """Both forms as fp32 tables on the host: the detector's (x / 255 - mean) / std and Sam.preprocess's (x - mean) / std."""
    mean, std = torch.tensor([123.675, 116.28, 103.53], device=dev).view(-1, 1, 1), torch.tensor([58.395, 57.12, 57.375], device=dev).view(-1, 1, 1)
    return {"unit": (lambda dt: ip.lut_unit_mean_std(gs.MEAN, gs.STD, dt, dev)), "sam": (lambda dt: ip.lut_sam(mean, std, dt))}


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("form", ["unit", "sam"])
def test_planar_output_equals_the_host_expression_and_the_pad_is_zero(dev, gold, dtype, form):
    """Into a canary-filled buffer with a guard on both sides: the image region is the lookup, the pad is zero, the guards are untouched.
    Pads: none, a few columns and rows (not a multiple of the 64 x 4 tile), and more than one tile."""
    make = luts32(dev)[form]
    lut = make(dtype)
    lut32 = make(torch.float32).cpu()
    assert torch.equal(lut.cpu(), lut32.to(dtype)), "the table of a 16-bit dtype is the fp32 table, cast"
    for case, pad in [(CASES[0], (0, 0)), (CASES[1], (3, 5)), (CASES[2], (70, 9)), (CASES[5], (1, 67)), (CASES[3], (2, 2))]:
        a = gold["in." + name(case)]
        oh, ow = case[2], case[3]
        hp, wp = oh + pad[0], ow + pad[1]
        for r in RESAMPLE:
            for B in (1, 2):
                imgs = np.stack([a, 255 - a])[:B]
                guard = 512
                frame = torch.full((B * 3 * hp * wp + 2 * guard,), CANARY, dtype=dtype, device=dev)
                out = frame[guard:guard + B * 3 * hp * wp]
                got = ops.image_prep(torch.from_numpy(imgs).to(dev), (oh, ow), r, lut=lut, pad_hw=(hp, wp), out=out)
                assert got.shape == (B, 3, hp, wp) and got.data_ptr() == out.data_ptr()
                assert torch.all(frame[:guard] == CANARY) and torch.all(frame[-guard:] == CANARY), "wrote outside the output"
                for b in range(B):
                    resized = gold[f"out.{name(case)}.{r}"] if b == 0 else ip.resize_reference(imgs[b], (ow, oh), r)
                    want = host_planar(resized, lut32, (hp, wp), dtype)
                    assert torch.equal(got[b].cpu(), want), (case, pad, r, B, b)
                    assert not got[b, :, oh:, :].any() and not got[b, :, :, ow:].any()
    # without out=, from a [H, W, 3] image: [3, Hpad, Wpad]
    a = gold["in." + name(CASES[0])]
    got = ops.image_prep(torch.from_numpy(a).to(dev), (23, 31), 2, lut=lut, pad_hw=(24, 40))
    assert got.shape == (3, 24, 40) and got.dtype == dtype
    assert torch.equal(got.cpu(), host_planar(gold[f"out.{name(CASES[0])}.2"], lut32, (24, 40), dtype))


def test_identity_sizes(dev, gold):
    """Neither axis changes: the uint8 result is the image, the planar one its lookup — the epilogue alone."""
    a = gold["in." + name(CASES[7])]                                                  # 90 x 120
    d = torch.from_numpy(a).to(dev)
    for r in RESAMPLE:
        assert torch.equal(ops.image_prep(d, (90, 120), r), d)
    lut = ip.lut_unit_mean_std(gs.MEAN, gs.STD, torch.float16, dev)
    got = ops.image_prep(d, (90, 120), 2, lut=lut, pad_hw=(96, 128))
    assert torch.equal(got.cpu(), host_planar(a, ip.lut_unit_mean_std(gs.MEAN, gs.STD, torch.float32, "cpu"), (96, 128), torch.float16))


def test_1024_to_800_equals_the_installed_pillow(dev):
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(11)
    a = rs.randint(0, 256, (1024, 1024, 3)).astype(np.uint8)
    a[:512] = np.where(rs.rand(512, 1024, 3) < 0.5, 0, 255).astype(np.uint8)
    d = torch.from_numpy(a).to(dev)
    for r in RESAMPLE:
        want = np.asarray(Image.fromarray(a).resize((800, 800), r))
        assert torch.equal(ops.image_prep(d, (800, 800), r).cpu(), torch.from_numpy(want))


def test_refusals(dev):
    good = torch.zeros(8, 9, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(L.OmgHipError, match="not contiguous"):
        ops.image_prep(torch.zeros(8, 3, 9, dtype=torch.uint8, device=dev).permute(0, 2, 1), (4, 4), 2)
    with pytest.raises(L.OmgHipError, match="torch.float32"):
        ops.image_prep(good.float(), (4, 4), 2)
    with pytest.raises(L.OmgHipError, match=r"\(8, 9, 4\)"):
        ops.image_prep(torch.zeros(8, 9, 4, dtype=torch.uint8, device=dev), (4, 4), 2)
    with pytest.raises(L.OmgHipError, match="cpu"):
        ops.image_prep(good.cpu(), (4, 4), 2)
    with pytest.raises(L.OmgHipError, match="ndarray"):
        ops.image_prep(np.zeros((8, 9, 3), np.uint8), (4, 4), 2)
    with pytest.raises(L.OmgHipError, match="LANCZOS"):
        ops.image_prep(good, (4, 4), 1)
    with pytest.raises(L.OmgHipError, match="unknown"):
        ops.image_prep(good, (4, 4), 7)
    lut = torch.zeros(3, 256, dtype=torch.float16, device=dev)
    with pytest.raises(L.OmgHipError, match="smaller"):
        ops.image_prep(good, (4, 4), 2, lut=lut, pad_hw=(3, 4))
    with pytest.raises(L.OmgHipError, match="lookup table"):
        ops.image_prep(good, (4, 4), 2, lut=lut[:, :255])
    with pytest.raises(L.OmgHipError, match="lookup table"):
        ops.image_prep(good, (4, 4), 2, pad_hw=(8, 8))


# ------------------------------------------------------------------------------------------------ the preprocessors' device branches
@pytest.fixture(scope="module")
def image():
    rs = np.random.RandomState(21)
    a = rs.randint(0, 256, (60, 84, 3)).astype(np.uint8)
    a[:20] = np.where(rs.rand(20, 84, 3) < 0.5, 0, 255).astype(np.uint8)
    return a


def test_resize_longest_side_on_the_device(dev, image):
    t = sa.ResizeLongestSide(128)
    want = t.apply_image(image)
    got = t.apply_image(torch.from_numpy(image).to(dev))
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want))
    with pytest.raises(L.OmgHipError, match="cuda uint8"):
        t.apply_image(torch.from_numpy(image))


def test_sam_predictor_set_image_on_the_device(dev, image):
    gold = np.load(os.path.join(HERE, "golden", "sam_vit_golden.npz"))
    gold = {k: gold[k] for k in gold.files}
    for dt in (torch.float16, torch.bfloat16):
        model = vt.narrow_model(gold, "d64", dt, dev)
        host, device = sa.SamPredictor(model), sa.SamPredictor(model)
        host.set_image(image)
        device.set_image(torch.from_numpy(image).to(dev))
        assert device.input_size == host.input_size and device.original_size == host.original_size and device.is_image_set
        assert torch.equal(device.features, host.features)
        device.set_image(torch.from_numpy(np.ascontiguousarray(image[..., ::-1])).to(dev), image_format="BGR")
        assert torch.equal(device.features, host.features)


def test_efficientvit_sam_predictor_on_the_device(dev, image):
    gold = np.load(os.path.join(HERE, "golden", "sam_golden.npz"))
    gold = {k: gold[k] for k in gold.files}
    model = sam_torch.narrow_model(gold, torch.float16, dev)
    side = model.image_size[1]
    for a in (image, np.ascontiguousarray(np.resize(image, (side // 2, side, 3)))):      # resized; the long side already fits
        r_host, x_host = model.preprocess(a)
        r_dev, x_dev = model.preprocess(torch.from_numpy(a).to(dev))
        assert torch.equal(r_dev.cpu(), torch.from_numpy(np.ascontiguousarray(r_host))) and x_dev.dtype == torch.float32
        assert torch.equal(x_dev.cpu(), x_host)
        host, device = hip_sam.EfficientViTSamPredictor(model), hip_sam.EfficientViTSamPredictor(model)
        host.set_image(a)
        device.set_image(torch.from_numpy(a).to(dev))
        assert device.input_size == host.input_size and device.original_size == host.original_size
        assert torch.equal(device.features, host.features)


@pytest.mark.parametrize("resample", RESAMPLE)
def test_dpt_image_processor_on_the_device(dev, image, resample):
    for kw in (dict(size={"height": 96, "width": 96}, keep_aspect_ratio=True, ensure_multiple_of=32, image_mean=[0.5, 0.4, 0.3], image_std=[0.5, 0.25, 0.2]),
               dict(size=48), dict(do_resize=False, do_normalize=False), dict(size=40, do_rescale=False)):
        p = hip_dpt.DPTImageProcessor(resample=resample, **kw)
        want = p(images=[image, image[::-1].copy()]).pixel_values
        got = p(images=[torch.from_numpy(image).to(dev), torch.from_numpy(image[::-1].copy()).to(dev)]).pixel_values
        assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got.cpu(), want), kw
        one = p(images=torch.from_numpy(image).to(dev)).pixel_values
        assert torch.equal(one.cpu(), want[:1])
    with pytest.raises(L.OmgHipError, match="LANCZOS"):
        hip_dpt.DPTImageProcessor(resample=1, size=48)(images=torch.from_numpy(image).to(dev))


def test_load_image_dino_on_the_device(dev, image):
    src, want = gs.load_image_dino(image, size=90, max_size=150)
    d = torch.from_numpy(image).to(dev)
    src_d, got = gs.load_image_dino(d, size=90, max_size=150)
    assert src_d.data_ptr() == d.data_ptr() and got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    assert torch.equal(gs.load_image_dino(d, size=90, max_size=150, dtype=torch.float16)[1].cpu(), want.half())


def test_to_uint8_hwc_on_the_device(dev):
    x = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(5)).half()
    want = (x.float().permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")
    assert torch.equal(ip.to_uint8_hwc(x.to(dev)).cpu(), torch.from_numpy(want))


def test_the_launches_capture_in_a_graph(dev, gold):
    """After one uncaptured call (the tables' upload) the resize and its epilogue replay from a graph with the same bits."""
    case = CASES[5]
    d = torch.from_numpy(gold["in." + name(case)]).to(dev)
    lut = ip.lut_unit_mean_std(gs.MEAN, gs.STD, torch.float16, dev)
    eager = ops.image_prep(d, (case[2], case[3]), 3, lut=lut, pad_hw=(104, 80))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops.image_prep(d, (case[2], case[3]), 3, lut=lut, pad_hw=(104, 80))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager)
