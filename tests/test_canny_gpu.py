"""GPU tests of the Canny kernels (csrc/canny.hip) against the numpy model of omg_amd/canny.py.  Every comparison is an equality: both
sides are integer arithmetic, and the hysteresis is a function of the state map alone whatever order the workgroups run in."""
import sys

import numpy as np
import pytest
import torch

from omg_amd import _lib, canny as cn, ops
from tests import _canny_cases as cc

pytestmark = pytest.mark.gpu

CANARY = 0xA5
BIG = (2 * cc.TH + 1, 2 * cc.TW + 1)


def framed(dev, n, lead):
    """A buffer of canaries with room for ``n`` bytes ``lead`` bytes in: (buffer, data pointer of the payload)."""
    buf = torch.full((lead + n + 64,), CANARY, dtype=torch.uint8, device=dev)
    return buf, buf.data_ptr() + lead


def frame_intact(buf, n, lead):
    return bool((buf[:lead] == CANARY).all()) and bool((buf[lead + n:] == CANARY).all())


def nms_framed(dev, imgs, low, high, lead_in=0, lead_out=64):
    """omg_canny_nms on [B, H, W, C] numpy images, input and output inside canary frames at the given byte offsets."""
    B, H, W, C = imgs.shape
    src, p_in = framed(dev, imgs.size, lead_in)
    src[lead_in:lead_in + imgs.size] = torch.from_numpy(imgs.reshape(-1)).to(dev)
    dst, p_out = framed(dev, B * H * W, lead_out)
    _lib.check(_lib.lib().omg_canny_nms(B, H, W, C, p_in, low, high, p_out, torch.cuda.current_stream().cuda_stream), "omg_canny_nms")
    torch.cuda.synchronize()
    assert frame_intact(dst, B * H * W, lead_out), "omg_canny_nms wrote outside its output"
    assert torch.equal(src[lead_in:lead_in + imgs.size].cpu(), torch.from_numpy(imgs.reshape(-1)))
    return dst[lead_out:lead_out + B * H * W].view(B, H, W).cpu().numpy()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw", cc.SIZES + cc.SIZES_C3_ALIGN, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nms_equals_the_model(dev, hw, C):
    for kind in cc.CONTENTS:
        a = cc.image(kind, hw[0], hw[1], C)
        for low, high in ((100, 200), (0, 2041)):
            got = nms_framed(dev, a[None], low, high)[0]
            assert np.array_equal(got, cn.nms_reference(a, low, high)), (kind, low, high)


def test_nms_of_a_batch_of_two_different_images(dev):
    for C in (1, 3):
        imgs = np.stack([cc.image("blur", *BIG, C), cc.image("stairs", *BIG, C)])
        got = nms_framed(dev, imgs, 100, 200)
        for b in range(2):
            assert np.array_equal(got[b], cn.nms_reference(imgs[b], 100, 200)), (C, b)
        assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("lead_in,lead_out", [(1, 61), (2, 62), (3, 63), (0, 66)])
def test_nms_at_every_byte_alignment_of_image_and_states(dev, lead_in, lead_out):
    """The first and last partial dwords of the image go byte by byte; a state row that is not dword aligned is stored byte by byte."""
    for C in (1, 3):
        for hw in ((5, 7), (cc.TH + 1, cc.TW + 4), BIG):
            a = cc.image("quant", hw[0], hw[1], C)
            got = nms_framed(dev, a[None], 100, 200, lead_in, lead_out)[0]
            assert np.array_equal(got, cn.nms_reference(a, 100, 200)), (C, hw)


def test_ops_canny_nms_takes_every_input_shape(dev):
    a = cc.image("blur", 21, 37, 3)
    want = cn.nms_reference(a, 100, 200)
    t = torch.from_numpy(a).to(dev)
    assert np.array_equal(ops.canny_nms(t, 100, 200).cpu().numpy(), want)
    assert np.array_equal(ops.canny_nms(t[None], 200.5, 100.9).cpu().numpy(), want[None])
    gray = t[:, :, 0].contiguous()
    want1 = cn.nms_reference(a[:, :, 0], 100, 200)
    assert np.array_equal(ops.canny_nms(gray, 100, 200).cpu().numpy(), want1)
    assert np.array_equal(ops.canny_nms(gray[:, :, None], 100, 200).cpu().numpy(), want1)


# ---------------------------------------------------------------------------------------------- hysteresis on state maps built directly
MAPS = cc.state_maps()
MAPS["random 0.41 161x321"] = cc.random_map(161, 321, 0.41)          # 11 x 6 tiles


@pytest.fixture(scope="module")
def hysteresis_refs():
    return {name: cn.hysteresis_reference(s) for name, s in MAPS.items()}


@pytest.mark.parametrize("name", list(MAPS))
def test_hysteresis_equals_the_model(dev, hysteresis_refs, name):
    s = torch.from_numpy(MAPS[name]).to(dev)
    got = ops.canny_hysteresis(s)
    again = ops.canny_hysteresis(s)
    assert np.array_equal(got.cpu().numpy(), hysteresis_refs[name]), name
    assert torch.equal(got, again)
    assert torch.equal(s.cpu(), torch.from_numpy(MAPS[name]))


def test_the_serpentine_comes_out_whole_or_not_at_all(dev, hysteresis_refs):
    got = ops.canny_hysteresis(torch.from_numpy(MAPS["serpentine"]).to(dev))
    assert int((got == 255).sum()) == 1155 and int((got != 0).sum()) == 1155
    assert not ops.canny_hysteresis(torch.from_numpy(MAPS["serpentine, no strong pixel"]).to(dev)).any()


def test_nothing_leaks_between_the_images_of_a_batch(dev):
    """Image 0's last row and image 1's first row would connect if the batch were one image."""
    H, W = cc.TH + 3, cc.TW + 5
    s = np.zeros((2, H, W), dtype=np.uint8)
    s[0, H - 1, :] = 1
    s[0, :, W - 1] = 1
    s[1, 0, :] = 1
    s[1, 0, 3] = 2
    s[1, :, 0] = 1
    want = np.stack([cn.hysteresis_reference(s[0]), cn.hysteresis_reference(s[1])])
    assert not want[0].any() and want[1].any()
    assert cn.hysteresis_reference(s.reshape(2 * H, W))[:H].any()        # as one image they do connect
    for form in (dict(), dict(channels=3), dict(out_dtype=torch.float32)):
        got = ops.canny_hysteresis(torch.from_numpy(s).to(dev), **form).cpu().numpy()
        if "channels" in form:
            assert np.array_equal(got, np.repeat(want[..., None], 3, axis=-1))
        elif form:
            assert got.dtype == np.float32 and np.array_equal(got, np.repeat(want[:, None], 3, axis=1) / np.float32(255))
        else:
            assert np.array_equal(got, want)
    # the other way round: the strong pixel in image 0 must not light image 1
    s2 = s[::-1].copy()
    got = ops.canny_hysteresis(torch.from_numpy(s2).to(dev)).cpu().numpy()
    assert np.array_equal(got, want[::-1])


def test_hysteresis_writes_inside_its_output_alone(dev):
    s = MAPS["random 0.41 33x129"]
    H, W = s.shape
    lib = _lib.lib()
    st = torch.from_numpy(s).to(dev)
    ws = torch.empty(int(lib.omg_canny_hysteresis_ws_bytes(1, H, W)), dtype=torch.uint8, device=dev)
    assert ws.numel() >= 5 * H * W
    for form, code, n in ((0, 0, H * W), (1, 0, 3 * H * W), (2, _lib.OMG_F16, 6 * H * W), (2, _lib.OMG_F32, 12 * H * W)):
        buf, p = framed(dev, n, 64)
        _lib.check(lib.omg_canny_hysteresis(1, H, W, st.data_ptr(), ws.data_ptr(), form, code, p, torch.cuda.current_stream().cuda_stream),
                   "omg_canny_hysteresis")
        torch.cuda.synchronize()
        assert frame_intact(buf, n, 64), (form, code)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("kind", cc.CONTENTS)
def test_canny_equals_the_model_in_all_three_output_forms(dev, kind):
    from PIL import Image
    from omg_amd import compat
    for C in (1, 3):
        for hw in ((3, 5), (cc.TH + 1, cc.TW - 1), BIG):
            a = cc.image(kind, hw[0], hw[1], C)
            want = cn.canny_reference(a, 100, 200)
            t = torch.from_numpy(a).to(dev)
            assert np.array_equal(ops.canny(t, 100, 200).cpu().numpy(), want), (C, hw)
            three = np.repeat(want[:, :, None], 3, axis=2)
            assert np.array_equal(ops.canny(t, 100, 200, channels=3).cpu().numpy(), three), (C, hw)
            cond = compat._cond_image_tensor(Image.fromarray(three), hw[0], hw[1])           # what a ControlNet is given: [1, 3, H, W] fp32
            for dt in (torch.float32, torch.float16, torch.bfloat16):
                got = ops.canny(t, 100, 200, out_dtype=dt)
                assert got.dtype == dt and got.shape == (3, hw[0], hw[1])
                assert torch.equal(got[None].cpu(), cond.to(dt)), (C, hw, dt)
    b = np.stack([cc.image(kind, *BIG, 3, seed=s) for s in (1, 2)])
    got = ops.canny(torch.from_numpy(b).to(dev), 100, 200).cpu().numpy()
    assert np.array_equal(got, np.stack([cn.canny_reference(b[0], 100, 200), cn.canny_reference(b[1], 100, 200)]))


def test_Canny_takes_numpy_and_tensors(dev):
    import omg_amd
    a = cc.image("blur", 40, 70, 3)
    want = cn.canny_reference(a, 100, 200)
    got = omg_amd.Canny(a, 100, 200)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(omg_amd.Canny(a[:, :, 0], 50.5, 150), cn.canny_reference(a[:, :, 0], 50, 150))
    assert np.array_equal(omg_amd.Canny(a[:, ::2], 100, 200), cn.canny_reference(np.ascontiguousarray(a[:, ::2]), 100, 200))    # a numpy view is copied
    t = omg_amd.Canny(torch.from_numpy(a).to(dev), 100, 200)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), want)


def test_canny_condition_pil_and_pt_agree(dev):
    from PIL import Image
    import omg_amd
    a = cc.image("blur", 48, 80, 3)
    want = cn.canny_reference(a, 100, 200)
    pil = omg_amd.canny_condition(Image.fromarray(a))
    assert pil.mode == "RGB" and pil.size == (80, 48) and np.array_equal(np.asarray(pil), np.repeat(want[:, :, None], 3, axis=2))
    pt = omg_amd.canny_condition(torch.from_numpy(a).to(dev), output="pt")
    assert pt.is_cuda and pt.dtype == torch.float32 and pt.shape == (1, 3, 48, 80)
    assert torch.equal(pt.cpu(), torch.from_numpy(np.asarray(pil).astype(np.float32) / 255.0).permute(2, 0, 1)[None])
    half = omg_amd.canny_condition(a, 100, 200, output="pt", dtype=torch.float16)
    assert half.dtype == torch.float16 and torch.equal(half.float(), pt)


def test_the_demos_get_cannyedge_runs_under_compat_install(dev):
    """gradio_demo/app.py:332 as it is written, with the stand-in cv2 of compat.install()."""
    from PIL import Image
    from omg_amd import compat
    try:
        import cv2 as real  # noqa: F401
        pytest.skip("a real cv2 is installed: compat.install() leaves it alone")
    except ImportError:
        pass
    saved_path = list(sys.path)
    try:
        compat.install()
        import cv2

        def get_cannyedge(image):
            image = np.array(image)
            image = cv2.Canny(image, 100, 200)
            image = image[:, :, None]
            image = np.concatenate([image, image, image], axis=2)
            canny_image = Image.fromarray(image)
            return canny_image

        a = cc.image("blur", 64, 96, 3)
        out = get_cannyedge(Image.fromarray(a))
    finally:
        compat.uninstall()
        sys.path[:] = saved_path
    assert np.array_equal(np.asarray(out), np.repeat(cn.canny_reference(a, 100, 200)[:, :, None], 3, axis=2))


def test_replay_from_a_graph_equals_eager(dev):
    a = torch.from_numpy(cc.image("blur", 70, 131, 3)).to(dev)
    b = torch.from_numpy(cc.image("stairs", 70, 131, 3)).to(dev)
    eager = {k: (ops.canny(x, 100, 200), ops.canny(x, 100, 200, out_dtype=torch.float16)) for k, x in (("a", a), ("b", b))}
    x = a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.canny(x, 100, 200)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e = ops.canny(x, 100, 200)
        p = ops.canny_hysteresis(ops.canny_nms(x, 100, 200), out_dtype=torch.float16)
    for k, src in (("a", a), ("b", b), ("a", a)):
        x.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(e, eager[k][0]) and torch.equal(p, eager[k][1]), k
    assert not torch.equal(eager["a"][0], eager["b"][0])


def test_refusals_on_the_device(dev):
    t = torch.zeros(8, 12, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.OmgHipError, match="not contiguous"):
        ops.canny_nms(t[:, ::2], 100, 200)
    with pytest.raises(_lib.OmgHipError, match="torch.float16"):
        ops.canny(t.half(), 100, 200)
    with pytest.raises(_lib.OmgHipError, match="C = 2"):
        ops.canny_nms(torch.zeros(8, 12, 2, dtype=torch.uint8, device=dev), 100, 200)
    with pytest.raises(_lib.OmgHipError, match="C = 4"):
        ops.canny(torch.zeros(2, 8, 12, 4, dtype=torch.uint8, device=dev), 100, 200)
    with pytest.raises(_lib.OmgHipError, match="NaN"):
        ops.canny(t, float("nan"), 200)
    s = torch.ones(8, 12, dtype=torch.uint8, device=dev)
    s[3, 4] = 7
    with pytest.raises(_lib.OmgHipError, match="holds the value 7"):
        ops.canny_hysteresis(s)
    with pytest.raises(_lib.OmgHipError, match="not contiguous"):
        ops.canny_hysteresis(torch.ones(8, 12, dtype=torch.uint8, device=dev).t())
    with pytest.raises(_lib.OmgHipError, match="channels=2"):
        ops.canny_hysteresis(torch.ones(8, 12, dtype=torch.uint8, device=dev), channels=2)
    with pytest.raises(_lib.OmgHipError, match="torch.int32"):
        ops.canny_hysteresis(torch.ones(8, 12, dtype=torch.uint8, device=dev), out_dtype=torch.int32)
    with pytest.raises(_lib.OmgHipError, match=r"\(4, 8, 12, 3\)|\[H, W\] or \[B, H, W\]"):
        ops.canny_hysteresis(torch.ones(4, 8, 12, 3, dtype=torch.uint8, device=dev))
