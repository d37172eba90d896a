"""omg_amd.GroundedSam on the GPU (-m gpu): the stage hand-off of ``--segment_type GroundingDINO`` with the image on the device,
against the host composition of the same modules written out here — ``torch.equal`` throughout.

The detector is tests/test_gdino_detector_gpu.py's (Swin ``w7``, the 128-wide BERT, encoder and head config "a", 70 queries) with
``size`` = that config's short side, so a 64 x 84 image becomes the backbone's 90 x 118 input; SAM is the narrow ``d64`` model of
tests/test_sam_vit_gpu.py (its 1024-wide encoder input is the largest piece).  The tokenizer is a stub.

``box_threshold`` is set from the scores of the host composition, read once: midway between two adjacent values, at least 1e-3 apart,
of the sorted scores that lie between the two captions' maxima — one caption then finds a box (several queries pass, so "the first in
query order" is not "the best") and the other finds none."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import os

from omg_amd import GroundedSam, bert as hip_bert, gdino as hip_gdino, gdino_decoder as hip, grounded_sam as gs, segment_anything as sa, swin as hip_swin
from tests import bert_torch as bt
from tests import gdino_decoder_torch as gd
from tests import gdino_torch as gt
from tests import sam_vit_torch as vt
from tests import swin_torch as st
from tests.test_gdino_detector_gpu import BERT

HERE = os.path.dirname(os.path.abspath(__file__))
CAPTIONS = ["Man", "tall woman."]
WORDS = {"man": 204, "tall": 371, "woman": 655}


class StubTokenizer:
    """[CLS] words '.' [SEP] from a three-word vocabulary, right padded with 0 to the longest."""

    def __call__(self, texts, padding="longest", return_tensors="pt"):
        rows = []
        for t in texts:
            assert t == t.lower().strip() and t.endswith("."), f"caption not normalised: {t!r}"
            rows.append([101] + [WORDS[w] for w in t[:-1].split()] + [1012, 102])
        T = max(len(r) for r in rows)
        ids = torch.tensor([r + [0] * (T - len(r)) for r in rows], dtype=torch.long)
        return {"input_ids": ids, "token_type_ids": torch.zeros_like(ids), "attention_mask": (ids != 0).long()}

    def decode(self, ids):
        inv = {v: k for k, v in WORDS.items()}
        inv[1012] = "."
        return " ".join(inv[int(i)] for i in ids)


def build_detector(dev, dt=torch.float16):
    scfg = st.small_cfg("w7")
    back = hip_swin.SwinBackbone(st.hf_config_dict(scfg), dtype=dt, device=dev)
    back.load_state_dict(st.seed_state(scfg, 41), strict=True)
    text = hip_bert.BertTextEncoder(bt.hf_config_dict(BERT), dtype=dt, device=dev)
    text.load_state_dict(bt.seed_state(BERT, 81), strict=True)
    ecfg = gt.small_cfg("a")
    ecfg.update(in_channels=list(back.channels), image=tuple(scfg["image"]), text_hidden=BERT["hidden"])
    enc = hip_gdino.GroundingDinoEncoder(ecfg, dtype=dt, device=dev)
    enc.load_state_dict(gt.seed_state(ecfg, 61), strict=True)
    dcfg = gd.small_cfg("a")
    head = hip.GroundingDinoDecoderHead(dcfg, dtype=dt, device=dev)
    head.load_state_dict(gd.seed_state(dcfg, 91), strict=True)
    return hip.GroundingDinoDetector(back, text, enc, head), min(scfg["image"])


class Counter:
    def __init__(self, obj, attr):
        self.n, self.obj, self.attr, self.fn = 0, obj, attr, getattr(obj, attr)
        setattr(obj, attr, self)

    def __call__(self, *a, **k):
        self.n += 1
        return self.fn(*a, **k)

    def restore(self):
        delattr(self.obj, self.attr)                 # the class's own method shows again


@pytest.fixture(scope="module")
def world(dev):
    """The models, the image, the host composition per caption (read once) and the threshold chosen from its scores."""
    from PIL import Image
    det, size = build_detector(dev)
    gold = np.load(os.path.join(HERE, "golden", "sam_vit_golden.npz"))
    sam_model = vt.narrow_model({k: gold[k] for k in gold.files}, "d64", torch.float16, dev)
    tok = StubTokenizer()
    rs = np.random.RandomState(33)
    image = rs.randint(0, 256, (64, 84, 3)).astype(np.uint8)
    image[16:40, 20:60] = np.where(rs.rand(24, 40, 3) < 0.5, 0, 255).astype(np.uint8)
    H, W = image.shape[:2]

    # ---- the host path per caption, as the parent's API allows it: PIL resize on the host, upload, detector
    ow, oh = gs.get_size_with_aspect_ratio((W, H), size, 1333)
    assert (oh, ow) == (90, 118)
    resized = np.asarray(Image.fromarray(image).resize((ow, oh), Image.BILINEAR))
    x = torch.from_numpy(np.array(resized)).permute(2, 0, 1).float().div(255)
    x = (x - torch.tensor(gs.MEAN)[:, None, None]) / torch.tensor(gs.STD)[:, None, None]
    outs = []
    for c in CAPTIONS:
        t = tok([gs.preprocess_caption(c)])
        outs.append(det(x[None].to(dev).half(), t["input_ids"].to(dev), t["token_type_ids"].to(dev), t["attention_mask"].to(dev)))
    scores = [o.logits.sigmoid().max(-1)[0][0].cpu() for o in outs]
    tops = [float(s.max()) for s in scores]
    hi = int(tops[1] > tops[0])
    lo_top, hi_top = tops[1 - hi], tops[hi]
    between = sorted({lo_top} | {float(v) for v in scores[hi] if lo_top < float(v) <= hi_top})
    gaps = [(a, b) for a, b in zip(between[:-1], between[1:]) if b - a >= 1e-3]
    print(f"maxima {tops}; {len(between)} scores between them, gaps of 1e-3 or more: {gaps[:4]}")
    assert gaps, f"no two adjacent scores between the captions' maxima {tops} are 1e-3 apart"
    threshold = 0.5 * (gaps[0][0] + gaps[0][1])

    host_pred = sa.SamPredictor(sam_model)
    expected = []
    for o in outs:
        boxes, _, _ = hip.detect(o, threshold, 0.25)[0]
        if boxes.shape[0] == 0:
            expected.append(None)
            continue
        host_pred.set_image(image)
        xyxy = gs.box_cxcywh_to_xyxy(boxes.cpu()) * torch.Tensor([W, H, W, H])
        prompts = host_pred.transform.apply_boxes_torch(xyxy, image.shape[:2]).to(dev)
        masks, _, _ = host_pred.predict_torch(point_coords=None, point_labels=None, boxes=prompts, multimask_output=False)
        expected.append(dict(mask=masks[0].squeeze(0), box=xyxy[0], kept=int(boxes.shape[0])))
    return dict(det=det, size=size, sam_model=sam_model, tok=tok, image=image, threshold=threshold, expected=expected, hi=hi, dev=dev)


def make(world):
    return GroundedSam(world["det"], sa.SamPredictor(world["sam_model"]), tokenizer=world["tok"], size=world["size"])


def test_the_threshold_splits_the_captions(world):
    e = world["expected"]
    assert e[world["hi"]] is not None and e[1 - world["hi"]] is None
    assert e[world["hi"]]["kept"] >= 1


def test_predict_masks_equals_the_host_composition(world):
    dev = world["dev"]
    g = make(world)
    image = torch.from_numpy(world["image"]).to(dev)
    swin, vit = Counter(world["det"].backbone, "forward"), Counter(world["sam_model"].image_encoder, "forward_features")
    try:
        masks, boxes, found = g.predict_masks(image, CAPTIONS, box_threshold=world["threshold"])
    finally:
        swin.restore()
        vit.restore()
    assert swin.n == 1 and vit.n == 1, "the backbone and SAM's image encoder run once for two captions"
    H, W = world["image"].shape[:2]
    assert masks.shape == (2, H, W) and masks.dtype == torch.bool and boxes.shape == (2, 4) and found.shape == (2,) and found.dtype == torch.bool
    assert masks.is_cuda and boxes.is_cuda and found.is_cuda
    assert found.tolist() == [e is not None for e in world["expected"]]
    e = world["expected"][world["hi"]]
    assert torch.equal(boxes[world["hi"]].cpu(), e["box"]), (boxes[world["hi"]].cpu(), e["box"])
    assert torch.equal(masks[world["hi"]], e["mask"])
    # a numpy image takes the same path after its upload
    m2, b2, f2 = g.predict_masks(world["image"], CAPTIONS, box_threshold=world["threshold"])
    assert torch.equal(m2, masks) and torch.equal(b2, boxes) and torch.equal(f2, found)


def test_batched_captions_equal_each_caption_alone(world):
    g = make(world)
    image = torch.from_numpy(world["image"]).to(world["dev"])
    masks, boxes, found = g.predict_masks(image, CAPTIONS, box_threshold=world["threshold"])
    for i, c in enumerate(CAPTIONS):
        m, b, f = g.predict_masks(image, [c], box_threshold=world["threshold"])
        assert torch.equal(f[0], found[i]) and torch.equal(b[0], boxes[i]) and torch.equal(m[0], masks[i]), c


def test_predict_mask_is_the_references_function(world):
    g = make(world)
    image = torch.from_numpy(world["image"]).to(world["dev"])
    hi = world["hi"]
    m = g.predict_mask(image, CAPTIONS[hi], box_threshold=world["threshold"])
    assert m.shape == world["image"].shape[:2] and torch.equal(m, world["expected"][hi]["mask"])
    assert g.predict_mask(image, CAPTIONS[1 - hi], box_threshold=world["threshold"]) is None


def test_graph_replay_equals_eager(world):
    dev = world["dev"]
    g = make(world)
    image = torch.from_numpy(world["image"]).to(dev)
    ids = world["tok"]([gs.preprocess_caption(c) for c in CAPTIONS])["input_ids"].to(dev)
    eager = g.predict_masks(image, ids, box_threshold=world["threshold"])
    text = g.predict_masks(image, CAPTIONS, box_threshold=world["threshold"])
    assert all(torch.equal(a, b) for a, b in zip(eager, text)), "input_ids and the captions they come from"
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g.predict_masks(image, ids, box_threshold=world["threshold"])           # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = g.predict_masks(image, ids, box_threshold=world["threshold"])
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(cap, eager):
        assert torch.equal(a, b)
    # another image through the same graph: the captured call reads the image's buffer
    other = torch.from_numpy(np.ascontiguousarray(world["image"][::-1])).to(dev)
    want = g.predict_masks(other, ids, box_threshold=world["threshold"])
    image.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(cap, want):
        assert torch.equal(a, b)


def test_predict_is_the_original_packages_function(world):
    """(boxes, scores, phrases) on the host for one caption, against detect / phrases on the same output."""
    dev = world["dev"]
    hi = world["hi"]
    _, x = gs.load_image_dino(torch.from_numpy(world["image"]).to(dev), size=world["size"])
    boxes, scores, found = gs.predict(world["det"], x, CAPTIONS[hi], world["threshold"], 0.0, tokenizer=world["tok"], device=dev)
    e = world["expected"][hi]
    assert not boxes.is_cuda and boxes.shape == (e["kept"], 4) and scores.shape == (e["kept"],) and len(found) == e["kept"]
    assert all("." not in p for p in found) and found[0] == gs.preprocess_caption(CAPTIONS[hi])[:-1]
    H, W = world["image"].shape[:2]
    assert torch.equal((gs.box_cxcywh_to_xyxy(boxes) * torch.Tensor([W, H, W, H]))[0], e["box"])
