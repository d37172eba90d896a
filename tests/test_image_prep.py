"""omg_amd/image_prep.py and the host side of omg_amd/grounded_sam.py (CPU, -m "not gpu"): the numpy model of Pillow's two-pass
fixed-point resize against the fixture of tests/golden/make_golden_image_prep.py and against the installed Pillow, facts about the
tables, the size rule and caption normalisation of the original GroundingDINO package, and to_uint8_hwc against the pipeline's numpy
line.  Every comparison is an equality."""
import os

import numpy as np
import pytest
import torch

from omg_amd import image_prep as ip
from omg_amd import grounded_sam as gs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_prep.npz")
# h, w -> oh, ow: down, up, 64 -> 3 rows with the width kept, everything into one pixel, one row, more than one block of 64 outputs,
# the height kept, and odd sizes both ways; the last is a segment beyond the horizontal kernel's LDS buffer
CASES = [(37, 53, 23, 31), (17, 19, 40, 33), (64, 48, 3, 48), (5, 7, 1, 1), (1, 9, 4, 20), (128, 96, 100, 75), (33, 33, 33, 20),
         (90, 120, 67, 89), (1, 4200, 1, 2)]
RESAMPLE = [ip.BILINEAR, ip.BICUBIC]


def name(case):
    h, w, oh, ow = case
    return f"{h}x{w}_{oh}x{ow}"


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("resample", RESAMPLE)
@pytest.mark.parametrize("case", CASES, ids=name)
def test_resize_reference_equals_the_fixture(gold, case, resample):
    a = gold["in." + name(case)]
    assert a.shape == (case[0], case[1], 3) and a.dtype == np.uint8
    want = gold[f"out.{name(case)}.{resample}"]
    got = ip.resize_reference(a, (case[3], case[2]), resample)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("resample", RESAMPLE)
@pytest.mark.parametrize("case", CASES, ids=name)
def test_resize_reference_equals_the_installed_pillow(gold, case, resample):
    Image = pytest.importorskip("PIL.Image")
    a = gold["in." + name(case)]
    want = np.asarray(Image.fromarray(a).resize((case[3], case[2]), resample))
    assert np.array_equal(ip.resize_reference(a, (case[3], case[2]), resample), want)


def test_the_fixture_exercises_both_ends_of_the_clip(gold):
    """Bicubic overshoot on the 0 / 255 half: some unclipped sums are below 0 and some above 255."""
    a = gold["in.128x96_100x75"].astype(np.int64)
    bounds, coeffs = ip.resize_tables(96, 75, ip.BICUBIC)
    lo = hi = False
    for xx in range(75):
        x0, n = bounds[xx]
        ss = ((1 << 21) + (a[:, x0:x0 + n] * coeffs[xx, :n][None, :, None].astype(np.int64)).sum(1)) >> 22
        lo, hi = lo or bool((ss < 0).any()), hi or bool((ss > 255).any())
    assert lo and hi


@pytest.mark.parametrize("resample", RESAMPLE)
def test_table_facts(resample):
    for i, o in [(53, 31), (19, 33), (64, 3), (7, 1), (1, 4), (9, 20), (1024, 800), (96, 75), (4200, 2)]:
        bounds, coeffs = ip.resize_tables(i, o, resample)
        S = 1 if resample == ip.BILINEAR else 2
        ksize = int(np.ceil(S * max(i / o, 1.0))) * 2 + 1
        assert bounds.shape == (o, 2) and coeffs.shape == (o, ksize) and bounds.dtype == np.int32 and coeffs.dtype == np.int32
        first, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
        assert (first >= 0).all() and (n >= 1).all() and (n <= ksize).all() and (first + n <= i).all()
        assert (np.diff(first) >= 0).all() and (np.diff(first + n) >= 0).all()          # the horizontal kernel's segment relies on it
        total = coeffs.astype(np.int64).sum(1)
        assert (np.abs(total - (1 << 22)) <= ksize).all(), (i, o, total)
        for xx in range(o):
            assert not coeffs[xx, n[xx]:].any()
    assert ip.resize_tables(64, 3, ip.BILINEAR)[1].shape[1] == 45


def test_other_filters_are_refused_by_name():
    for code, word in [(0, "NEAREST"), (1, "LANCZOS"), (4, "BOX"), (5, "HAMMING")]:
        with pytest.raises(ValueError, match=word):
            ip.resize_tables(8, 4, code)
    with pytest.raises(ValueError, match="unknown"):
        ip.resize_reference(np.zeros((4, 4, 3), np.uint8), (2, 2), 9)


def test_size_rule_of_the_original_package():
    assert gs.get_size_with_aspect_ratio((1024, 1024)) == (800, 800)
    assert gs.get_size_with_aspect_ratio((1024, 768)) == (1066, 800)
    assert gs.get_size_with_aspect_ratio((2000, 500)) == (1332, 333)
    assert gs.get_size_with_aspect_ratio((768, 1024)) == (800, 1066)
    assert gs.get_size_with_aspect_ratio((800, 1000)) == (800, 1000)                  # the short side is already the size
    assert gs.get_size_with_aspect_ratio((84, 64), size=90) == (118, 90)


def test_caption_normalisation():
    assert gs.preprocess_caption("  Man ") == "man."
    assert gs.preprocess_caption("woman.") == "woman."
    assert gs.preprocess_caption("A Dog . ") == "a dog ."


def test_box_cxcywh_to_xyxy():
    b = torch.tensor([[0.5, 0.25, 0.5, 0.125], [0.75, 0.5, 0.25, 1.0]])
    assert torch.equal(gs.box_cxcywh_to_xyxy(b), torch.tensor([[0.25, 0.1875, 0.75, 0.3125], [0.625, 0.0, 0.875, 1.0]]))


def test_to_uint8_hwc_is_the_pipelines_numpy_line():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 9, 11, generator=g)
    x[0, :, 0, :4] = torch.tensor([0.0, 1.0, 0.5, 127.5 / 255])
    for t in (x, x.half(), x.bfloat16()):
        want = (t.float().permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")
        got = ip.to_uint8_hwc(t)
        assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.numpy(), want)
        assert np.array_equal(ip.to_uint8_hwc(t[1]).numpy(), want[1])
    with pytest.raises(ValueError):
        ip.to_uint8_hwc(torch.zeros(2, 4, 5, 5))


def test_lookup_tables_are_the_host_expressions():
    u8 = np.arange(256, dtype=np.uint8)
    lut = ip.lut_unit_mean_std(gs.MEAN, gs.STD, torch.float32, "cpu")
    x = torch.from_numpy(u8)[None, None].expand(3, 1, 256).float().div(255)
    want = (x - torch.tensor(gs.MEAN)[:, None, None]) / torch.tensor(gs.STD)[:, None, None]
    assert torch.equal(lut, want[:, 0]) and torch.equal(ip.lut_unit_mean_std(gs.MEAN, gs.STD, torch.float16, "cpu"), want[:, 0].half())
    mean, std = [0.5, 0.4, 0.3], [0.5, 0.25, 0.2]
    a = np.repeat(u8[:, None], 3, 1).astype(np.float32) * np.float32(1 / 255)
    a = (a - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    assert np.array_equal(ip.lut_numpy_rescale_mean_std(1 / 255, mean, std, torch.float32, "cpu").numpy(), a.T)
    assert np.array_equal(ip.lut_numpy_rescale_mean_std(None, None, std, torch.float32, "cpu").numpy(), np.repeat(u8[None], 3, 0).astype(np.float32))


def test_load_image_dino_on_the_host():
    Image = pytest.importorskip("PIL.Image")
    a = np.random.RandomState(2).randint(0, 256, (64, 84, 3)).astype(np.uint8)
    src, x = gs.load_image_dino(Image.fromarray(a), size=90, max_size=150)
    assert np.array_equal(src, a) and x.shape == (3, 90, 118) and x.dtype == torch.float32
    r = ip.resize_reference(a, (118, 90), ip.BILINEAR)
    lut = ip.lut_unit_mean_std(gs.MEAN, gs.STD, torch.float32, "cpu")
    want = torch.stack([lut[c][torch.from_numpy(r[..., c].astype(np.int64))] for c in range(3)])
    assert torch.equal(x, want)
