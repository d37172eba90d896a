"""omg_amd.GroundingDinoDetector with every part on the HIP kernels (-m gpu): SwinBackbone -> BertTextEncoder -> GroundingDinoEncoder ->
GroundingDinoDecoderHead on seeded parts, from pixels and token ids to logits and boxes, captured in ONE torch.cuda.graph — against the
chain of the four plain-torch oracles (tests/swin_torch.py, bert_torch.py, gdino_torch.py, gdino_decoder_torch.py).

The bound is composed as tests/test_gdino_gpu.py::test_chain_from_the_swin_backbone composes it: rms error / rms of the oracle chain's
output within 2 x (FACTOR of the neighbouring files) the same figure of the chain of the four 16-bit twins.  The selection's ORDER is the
module's own (tests/test_gdino_decoder_gpu.py::test_own_selection_picks_the_librarys_set says why it matters), so the oracle and the
twin run on the proposals the module selected.

Measured on an MI355X (HIP figure / twin figure; the twin's own figure in brackets): the text encoder's output 0.92 (1.1e-3), the logits
1.19 (1.3e-2), the boxes 1.01 (2.7e-3).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import bert as hip_bert
from omg_amd import gdino as hip_gdino
from omg_amd import gdino_decoder as hip
from omg_amd import swin as hip_swin
from tests import bert_torch as bt
from tests import gdino_decoder_torch as gd
from tests import gdino_torch as gt
from tests import swin_torch as st

FACTOR = 2.0
BERT = dict(hidden=128, heads=2, inter=264, layers=2, vocab=1100, positions=64, types=2, eps=1e-12)


def figure(got, ref):
    keep = torch.isfinite(ref)
    return gd.rel_rms(got[keep], ref[keep])


def test_the_whole_detector_call_in_one_graph(dev):
    dt = torch.float16
    scfg = st.small_cfg("w7")
    ssd = st.seed_state(scfg, 41)
    x = torch.from_numpy(st.seeded_input(9, 2, *scfg["image"]).astype(np.float32) / 8.0)
    back = hip_swin.SwinBackbone(st.hf_config_dict(scfg), dtype=dt, device=dev)
    back.load_state_dict(ssd, strict=True)
    bsd = bt.seed_state(BERT, 81)
    text = hip_bert.BertTextEncoder(bt.hf_config_dict(BERT), dtype=dt, device=dev)
    text.load_state_dict(bsd, strict=True)
    ecfg = gt.small_cfg("a")
    ecfg.update(in_channels=list(back.channels), image=tuple(scfg["image"]), text_hidden=BERT["hidden"])
    esd = gt.seed_state(ecfg, 61)
    enc = hip_gdino.GroundingDinoEncoder(ecfg, dtype=dt, device=dev)
    enc.load_state_dict(esd, strict=True)
    dcfg = gd.small_cfg("a")
    dsd = gd.seed_state(dcfg, 91)
    head = hip.GroundingDinoDecoderHead(dcfg, dtype=dt, device=dev)
    head.load_state_dict(dsd, strict=True)
    det = hip.GroundingDinoDetector(back, text, enc, head)
    assert isinstance(det.text_backbone, hip_bert.BertTextEncoder)

    inp = bt.seeded_ids(BERT, 23, 7)
    ids, types = inp["input_ids"][:2], inp["token_type_ids"][:2]
    token_mask = ids != 0
    args = [x.to(dev), ids.to(dev), types.to(dev), token_mask.long().to(dev)]
    eager = det(*args)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        det(*args)                                   # warm-up off the default stream: workspaces, packed weights
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = det(*args)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.logits, eager.logits) and torch.equal(cap.pred_boxes, eager.pred_boxes)
    assert torch.equal(cap.topk_proposals, eager.topk_proposals)

    topk = cap.topk_proposals.cpu()
    mask, pos = inp["attention_mask"][:2], inp["position_ids"][:2]

    def chain(twin):
        r = (lambda sd: {k: v.to(twin).float() for k, v in sd.items()}) if twin is not None else (lambda sd: sd)
        kw = dict(twin=twin) if twin is not None else {}
        with torch.no_grad():
            fm = [f.float() for f in st.forward(r(ssd), scfg, x, **kw)["feature_maps"]]
            t = bt.forward(r(bsd), BERT, ids, mask, types, pos, **kw)[-1]
            e = gt.forward(r(esd), ecfg, fm, None, t, token_mask, mask, pos, **kw)
            d = gd.forward(r(dsd), dcfg, e["vision_states"][-1], e["text_states"][-1], e["mask_flatten"], token_mask, e["spatial"],
                           e["valid_ratios"], topk_proposals=topk, **kw)
        return dict(text=t, logits=d["logits"][-1], pred_boxes=d["pred_boxes"][-1])

    ref, tw = chain(None), chain(dt)
    got = dict(text=det.text_backbone(ids.to(dev), mask.to(dev), types.to(dev), pos.to(dev)).float().cpu(),
               logits=cap.logits.cpu(), pred_boxes=cap.pred_boxes.cpu())
    assert torch.equal(torch.isneginf(got["logits"]), torch.isneginf(ref["logits"])), "exact -inf pattern"
    for k in ("text", "logits", "pred_boxes"):
        e, t = figure(got[k], ref[k]), figure(tw[k], ref[k])
        print(f"detector chain {k}: rms error / rms {e:.3e}, twin {t:.3e}, ratio {e / t:.2f}")
    for k in ("text", "logits", "pred_boxes"):
        e, t = figure(got[k], ref[k]), figure(tw[k], ref[k])
        assert e <= FACTOR * t, (k, e, t)
