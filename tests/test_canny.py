"""CPU tests (-m "not gpu") of the numpy model of cv2.Canny in omg_amd/canny.py — the specification the kernels of csrc/canny.hip are held to
in tests/test_canny_gpu.py — and of the public layer's refusals.  Every comparison is an equality.  The model is written from OpenCV's
published algorithm; where ``cv2`` can be imported the last test pins it against the real thing, elsewhere that test skips."""
import sys

import numpy as np
import pytest
import torch

from omg_amd import _lib, canny as cn, ops
from tests import _canny_cases as cc


def step_image():
    a = np.zeros((8, 8), dtype=np.uint8)
    a[:, 4:] = 255
    return a


def test_a_vertical_step_gives_column_3_and_nothing_else():
    """Columns 3 and 4 both have mag 1020; column 3 passes (> left, >= right), column 4 does not."""
    a = step_image()
    dx, dy = cn.sobel_reference(a)
    assert (dx[:, 3:5, 0] == 1020).all() and not dx[:, [0, 1, 2, 5, 6, 7], 0].any() and not dy.any()
    want = np.zeros((8, 8), dtype=np.uint8)
    want[:, 3] = 255
    assert np.array_equal(cn.canny_reference(a, 100, 200), want)
    assert np.array_equal(cn.nms_reference(a, 100, 200), want // 255 * 2)


def test_a_horizontal_step_gives_row_3_and_nothing_else():
    want = np.zeros((8, 8), dtype=np.uint8)
    want[3, :] = 255
    assert np.array_equal(cn.canny_reference(step_image().T.copy(), 100, 200), want)


def test_gradients_equal_scipys_correlation_on_the_nearest_border():
    ndi = pytest.importorskip("scipy.ndimage")
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    for kind in cc.CONTENTS:
        a = cc.image(kind, 13, 17, 3)
        dx, dy = cn.sobel_reference(a)
        for c in range(3):
            plane = a[:, :, c].astype(np.int32)
            assert np.array_equal(dx[:, :, c], ndi.correlate(plane, kx, mode="nearest")), kind
            assert np.array_equal(dy[:, :, c], ndi.correlate(plane, kx.T, mode="nearest")), kind


def hysteresis_by_label(state):
    ndi = pytest.importorskip("scipy.ndimage")
    lab, n = ndi.label(state > 0, structure=np.ones((3, 3), dtype=int))
    strong = np.zeros(n + 1, dtype=bool)
    strong[np.unique(lab[state == 2])] = True
    strong[0] = False
    return (strong[lab] * 255).astype(np.uint8)


def test_hysteresis_equals_scipys_labelling_with_the_3x3_structure():
    for name, s in cc.state_maps().items():
        assert np.array_equal(cn.hysteresis_reference(s), hysteresis_by_label(s)), name


def test_the_hand_made_state_maps_are_what_they_claim():
    s = cc.serpentine(33, 67)
    assert int((s > 0).sum()) == 1155 and int((s == 2).sum()) == 1
    assert int(cn.hysteresis_reference(s).sum()) == 1155 * 255
    assert not cn.hysteresis_reference(cc.serpentine(33, 67, strong=False)).any()
    H, W = 2 * cc.TH + 1, 2 * cc.TW + 1
    d = cc.diagonal(H, W)
    assert d[cc.TH - 1, cc.TW - 1] and d[cc.TH, cc.TW] and (d.sum(axis=1) <= 2).all() and cn.hysteresis_reference(d).sum() == 255 * (d > 0).sum()
    t = cn.hysteresis_reference(cc.two_components(H, W))
    assert t[:, :cc.TW].all() and not t[:, cc.TW:].any()
    sp = cc.spiral(H, W)
    assert cn.hysteresis_reference(sp).sum() == 255 * (sp > 0).sum() and (sp > 0).sum() > H * W // 3


def nms_by_loops(image, low, high, order=(0, 1, 2)):
    """The specification once more, pixel by pixel in Python integers; ``order``: the sequence in which channels are tried (a later one
    must be strictly larger to win)."""
    a = image.astype(int)
    H, W, C = a.shape
    px = lambda y, x, c: a[min(max(y, 0), H - 1), min(max(x, 0), W - 1), c]
    g = np.zeros((H + 2, W + 2, 3), dtype=int)          # mag, dx, dy with a zero frame
    for y in range(H):
        for x in range(W):
            best = None
            for c in order[:C]:
                dx = (px(y - 1, x + 1, c) + 2 * px(y, x + 1, c) + px(y + 1, x + 1, c)) - (px(y - 1, x - 1, c) + 2 * px(y, x - 1, c) + px(y + 1, x - 1, c))
                dy = (px(y + 1, x - 1, c) + 2 * px(y + 1, x, c) + px(y + 1, x + 1, c)) - (px(y - 1, x - 1, c) + 2 * px(y - 1, x, c) + px(y - 1, x + 1, c))
                if best is None or abs(dx) + abs(dy) > best[0]:
                    best = (abs(dx) + abs(dy), dx, dy)
            g[y + 1, x + 1] = best
    out = np.zeros((H, W), dtype=np.uint8)
    hit = set()
    for y in range(1, H + 1):
        for x in range(1, W + 1):
            m, dx, dy = (int(v) for v in g[y, x])
            if m <= low:
                continue
            ax, ay = abs(dx), abs(dy) << 15
            t22 = ax * 13573
            t67 = t22 + (ax << 16)
            if ay < t22:
                keep, case = m > g[y, x - 1, 0] and m >= g[y, x + 1, 0], 0
            elif ay > t67:
                keep, case = m > g[y - 1, x, 0] and m >= g[y + 1, x, 0], 1
            elif (dx ^ dy) >= 0:
                keep, case = m > g[y - 1, x - 1, 0] and m > g[y + 1, x + 1, 0], 2
            else:
                keep, case = m > g[y - 1, x + 1, 0] and m > g[y + 1, x - 1, 0], 3
            hit.add(case)
            if keep:
                out[y - 1, x - 1] = 2 if m > high else 1
    return out, hit


@pytest.mark.parametrize("kind", cc.CONTENTS)
@pytest.mark.parametrize("C", [1, 3])
def test_nms_equals_the_pixel_by_pixel_loops(kind, C):
    a = cc.image(kind, 19, 23, C)
    want, hit = nms_by_loops(a, 100, 200)
    assert np.array_equal(cn.nms_reference(a, 100, 200), want)
    if kind in ("blur", "quant", "noise"):
        assert hit == {0, 1, 2, 3}, hit                 # every direction case


def test_the_image_cases_reach_what_they_are_for():
    big = {k: cn.nms_reference(cc.image(k, 2 * cc.TH + 1, 2 * cc.TW + 1, 1), 100, 200) for k in cc.CONTENTS}
    weak, strong = int((big["blur"] == 1).sum()), int((big["blur"] == 2).sum())
    assert strong >= 10 and weak >= 5 * strong, (weak, strong)
    assert (big["quant"] == 1).any() and (big["quant"] == 2).any() and (big["stairs"] == 1).any() and (big["stairs"] == 2).any()
    assert not (big["noise"] == 1).sum() > 0.02 * (big["noise"] == 2).sum()
    dx, dy = cn.sobel_reference(cc.image("checker", 33, 129, 1))
    assert int((np.abs(dx) + np.abs(dy)).max()) == 1530         # the largest |dx| + |dy| of a 3x3 Sobel pair on bytes (2040 bounds it)
    # ties on every side: equal magnitudes left / right / above / below / on both diagonals of a candidate
    for k in ("quant", "stairs"):
        dx, dy = cn.sobel_reference(cc.image(k, 33, 129, 1))
        m = (np.abs(dx) + np.abs(dy))[:, :, 0]
        c = m[1:-1, 1:-1]
        for oy, ox in ((0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (1, 1), (-1, 1), (1, -1)):
            assert ((c > 100) & (c == m[1 + oy:m.shape[0] - 1 + oy, 1 + ox:m.shape[1] - 1 + ox])).any(), (k, oy, ox)


def test_a_gray_image_stacked_three_times_gives_the_gray_images_states():
    for kind in cc.CONTENTS:
        a = cc.image(kind, 17, 21, 1)
        want = cn.nms_reference(a, 100, 200)
        assert np.array_equal(cn.nms_reference(a[:, :, 0], 100, 200), want)
        assert np.array_equal(cn.nms_reference(np.repeat(a, 3, axis=2), 100, 200), want)


def test_on_a_tie_between_channels_the_lowest_index_wins():
    """(a, a, b) and (a, b, a) try a before b, (b, a, a) tries b first: the model equals the loops that try channels in that order, and the
    order matters on this image (equal magnitudes with different directions)."""
    img = cc.image("quant", 19, 23, 3, seed=3)
    a, b = img[:, :, 0], img[:, :, 1]
    aab, aba, baa = (np.stack(p, axis=2) for p in ((a, a, b), (a, b, a), (b, a, a)))
    a_first = cn.nms_reference(aab, 60, 120)
    assert np.array_equal(a_first, cn.nms_reference(aba, 60, 120))
    assert np.array_equal(a_first, nms_by_loops(np.stack((a, b), axis=2), 60, 120, order=(0, 1))[0])
    b_first = cn.nms_reference(baa, 60, 120)
    assert np.array_equal(b_first, nms_by_loops(np.stack((a, b), axis=2), 60, 120, order=(1, 0))[0])
    assert not np.array_equal(a_first, b_first)


def test_threshold_handling():
    a = cc.image("blur", 33, 65, 3)
    ref = cn.canny_reference(a, 100, 200)
    assert ref.any() and not ref.all()
    assert np.array_equal(cn.canny_reference(a, 200, 100), ref)                     # swapped
    assert np.array_equal(cn.canny_reference(a, 100.7, 200.9), ref)                 # floored
    assert cn.thresholds(100.7, 200.2) == (100, 200) and cn.thresholds(200, 100) == (100, 200)
    low0 = cn.nms_reference(a, 0, 200)
    assert np.array_equal(low0, nms_by_loops(a, 0, 200)[0]) and (low0 > 0).sum() > (cn.nms_reference(a, 100, 200) > 0).sum()
    assert np.array_equal(cn.canny_reference(a, -5, 200), cn.canny_reference(a, 0, 200))
    for high in (2040, 2041, 1e9):
        assert not cn.canny_reference(cc.image("checker", 33, 65, 3), 100, high).any()
    assert cn.canny_reference(cc.image("checker", 33, 65, 3), 100, 1529).any()
    with pytest.raises(ValueError, match="NaN"):
        cn.thresholds(float("nan"), 1)


def test_the_model_refuses_what_it_does_not_cover():
    for bad in (np.zeros((4, 4), dtype=np.float32), np.zeros((4, 4, 2), dtype=np.uint8), np.zeros((4, 4, 4), dtype=np.uint8),
                np.zeros((2, 4, 4, 3), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            cn.canny_reference(bad, 100, 200)
    with pytest.raises(ValueError, match="state map"):
        cn.hysteresis_reference(np.full((3, 3), 3, dtype=np.uint8))


def test_refusals_by_name():
    a = np.zeros((8, 8, 3), dtype=np.uint8)
    with pytest.raises(_lib.OmgHipError, match="apertureSize=5"):
        cn.Canny(a, 100, 200, None, 5)
    with pytest.raises(_lib.OmgHipError, match="L2gradient"):
        cn.Canny(a, 100, 200, L2gradient=True)
    with pytest.raises(_lib.OmgHipError, match="edges"):
        cn.Canny(a, 100, 200, np.zeros((8, 8), dtype=np.uint8))
    with pytest.raises(_lib.OmgHipError, match="float32"):
        cn.Canny(a.astype(np.float32), 100, 200)
    with pytest.raises(_lib.OmgHipError, match="output='svg'"):
        cn.canny_condition(a, output="svg")
    # the ops: cpu tensors, other dtypes, non-contiguous input, C not in {1, 3}; all before anything touches a device
    t = torch.zeros(8, 8, 3, dtype=torch.uint8)
    for fn in (lambda x: ops.canny_nms(x, 100, 200), lambda x: ops.canny(x, 100, 200), lambda x: cn.Canny(x, 100, 200)):
        with pytest.raises(_lib.OmgHipError, match="on cpu"):
            fn(t)
    with pytest.raises(_lib.OmgHipError, match="on cpu"):
        ops.canny_hysteresis(t[:, :, 0].contiguous())
    with pytest.raises(_lib.OmgHipError, match="ndarray"):
        ops.canny_nms(a, 100, 200)
    meta = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="meta")
    with pytest.raises(_lib.OmgHipError, match="torch.uint8 .* on meta"):
        ops.canny_nms(meta, 100, 200)


def test_the_package_exports_the_public_names():
    import omg_amd
    assert omg_amd.Canny is cn.Canny and omg_amd.canny_condition is cn.canny_condition
    assert "Canny" in omg_amd.__all__ and "canny_condition" in omg_amd.__all__


def test_the_stand_in_cv2_resolves_canny_to_ours_and_nothing_else():
    from omg_amd import compat
    if "cv2" not in sys.modules:
        try:
            import cv2  # noqa: F401
            pytest.skip("a real cv2 is installed: compat.install() leaves it alone")
        except ImportError:
            pass
    saved_path = list(sys.path)
    try:
        compat.install()
        import cv2
        assert vars(cv2).get("__omg_amd_alias__") and cv2.Canny is cn.Canny
        for name in ("cvtColor", "COLOR_RGB2BGR", "GaussianBlur"):
            with pytest.raises(_lib.OmgHipError, match="cv2"):
                getattr(cv2, name)
    finally:
        compat.uninstall()
        sys.path[:] = saved_path
    assert "cv2" not in sys.modules


def test_the_model_equals_the_real_cv2():
    """Skips where OpenCV is not installed — the model is unpinned against it there — and pins it wherever the package exists."""
    cv2 = pytest.importorskip("cv2")
    if vars(cv2).get("__omg_amd_alias__"):
        pytest.skip("cv2 is the stand-in of compat.install()")
    for kind in cc.CONTENTS:
        for C in (1, 3):
            for h, w in cc.SIZES + cc.SIZES_C3_ALIGN:
                a = cc.image(kind, h, w, C)
                for t1, t2 in ((100, 200), (200, 100), (100.7, 200.2), (0, 50), (30, 2040)):
                    assert np.array_equal(cn.canny_reference(a, t1, t2), cv2.Canny(a if C == 3 else a[:, :, 0], t1, t2)), (kind, C, h, w, t1, t2)
