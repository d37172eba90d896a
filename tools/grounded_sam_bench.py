#!/usr/bin/env python
"""The stage hand-off of ``--segment_type GroundingDINO`` at full width — Swin-B, BERT-base, the 6 + 6 layer GroundingDINO encoder and
head (900 queries), SAM vit_h; seeded synthetic weights, fp16 — on one 1024 x 1024 image and the captions "man." and "woman.":

  (a) the host path, as the API allowed it before omg_amd.GroundedSam, once per caption: PIL resize on the host, normalise, upload,
      GroundingDinoDetector, ``detect``, the first kept box, ``SamPredictor.set_image`` on the numpy image (PIL resize on the host),
      ``predict_torch`` on that box alone (the reference decodes every kept box and keeps the first mask; decoding one is the
      least the host path can do and what (b) does) — so Swin-B and SAM's ViT-H run twice;
  (b) ``GroundedSam.predict_masks`` on the cuda uint8 image, eager;
  (c) the same call replayed from one ``torch.cuda.graph``;
  (d) the resize alone at 1024 x 1024 -> 800 x 800: ops.image_prep's launches to the detector's fp16 input against PIL's resize, the
      normalisation and the upload on the host.

    python tools/grounded_sam_bench.py [--log profiles/grounded_sam_bench.log] [--calls 5] [--timeout 900]

2 warm-up calls of each path, then two interleaved rounds of ``--calls`` synchronised calls each; per round the median is reported.
The box threshold is put below the best score of each caption on these random weights, so that both paths decode a box.  The last
lines say whether (b) and (c) are no slower than (a), and the device side of (d) no slower than its host side, in both rounds; the tool
exits with status 1 where one of them is not.  The tool ends itself after ``--timeout`` seconds.
"""
import argparse
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bert_bench
import gdino_bench
import gdino_decoder_bench
import sam_vit_bench
import swin_bench
from omg_amd import GroundedSam, bert, gdino, gdino_decoder, grounded_sam as gs, image_prep, ops, segment_anything as sa, swin

IDS = {"man.": [101, 2158, 1012, 102], "woman.": [101, 2450, 1012, 102]}       # bert-base-uncased


class Tokenizer:
    def __call__(self, texts, padding="longest", return_tensors="pt"):
        ids = torch.tensor([IDS[t] for t in texts], dtype=torch.long)
        return {"input_ids": ids, "token_type_ids": torch.zeros_like(ids), "attention_mask": torch.ones_like(ids)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rounds(fns, calls, n_rounds=2):
    out = []
    for _ in range(n_rounds):
        ts = [[] for _ in fns]
        for _ in range(calls):
            for t, f in zip(ts, fns):
                t.append(timed(f))
        out.append([statistics.median(t) for t in ts])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=900)
    a = ap.parse_args()
    signal.alarm(a.timeout)
    from PIL import Image
    dev = torch.device("cuda:0")
    dt = torch.float16
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"GroundingDINO (Swin-B, BERT-base, 6 + 6 layers, 900 queries) + SAM vit_h, fp16, seeded weights, one 1024 x 1024 image, captions "
         f"'man.' and 'woman.', {torch.cuda.get_device_name(0)}; medians of {a.calls} synchronised calls, two interleaved rounds")
    back = swin.SwinBackbone(swin_bench.SWIN_B, dtype=dt, device=dev)
    swin_bench.seed_model(back, 11)
    text = bert.BertTextEncoder(bert_bench.CFG, dtype=dt, device=dev)
    text.load_state_dict(bert_bench.seed_state(text, 12), strict=True)
    ecfg = dict(gdino_bench.CFG, in_channels=list(back.channels))
    enc = gdino.GroundingDinoEncoder(ecfg, dtype=dt, device=dev)
    gdino_bench.seed_model(enc, 13)
    head = gdino_decoder.GroundingDinoDecoderHead(gdino_decoder_bench.CFG, dtype=dt, device=dev)
    gdino_decoder_bench.seed_model(head, 14)
    det = gdino_decoder.GroundingDinoDetector(back, text, enc, head)
    sam_model = sa.build_sam_vit_h(device=dev)
    sam_vit_bench.seed_model(sam_model, 15)
    tok = Tokenizer()
    captions = ["man.", "woman."]
    rs = np.random.RandomState(0)
    image = rs.randint(0, 256, (1024, 1024, 3)).astype(np.uint8)
    image_d = torch.from_numpy(image).to(dev)
    H, W = image.shape[:2]
    mean, std = torch.tensor(gs.MEAN)[:, None, None], torch.tensor(gs.STD)[:, None, None]
    host_pred = sa.SamPredictor(sam_model)
    g = GroundedSam(det, sa.SamPredictor(sam_model), tokenizer=tok)
    ids = tok(captions)["input_ids"].to(dev)

    def host_input():
        r = np.array(Image.fromarray(image).resize((800, 800), Image.BILINEAR))
        x = torch.from_numpy(r).permute(2, 0, 1).float().div(255)
        return ((x - mean) / std).to(dev).to(dt)

    with torch.no_grad():
        scores = det(host_input()[None].expand(2, -1, -1, -1).contiguous(), ids).logits.sigmoid().max(-1)[0]
    threshold = float(scores.max(-1)[0].min()) * 0.999
    emit(f"box_threshold {threshold:.4f} (just below the smaller of the two captions' best scores): "
         f"{[int(v) for v in (scores > threshold).sum(-1)]} of {scores.shape[1]} queries pass")

    @torch.no_grad()
    def path_a():
        out = []
        for c in captions:
            t = tok([c])
            o = det(host_input()[None], t["input_ids"].to(dev), t["token_type_ids"].to(dev), t["attention_mask"].to(dev))
            boxes, _, _ = gdino_decoder.detect(o, threshold, 0.25)[0]
            host_pred.set_image(image)
            xyxy = gs.box_cxcywh_to_xyxy(boxes.cpu()) * torch.Tensor([W, H, W, H])
            prompts = host_pred.transform.apply_boxes_torch(xyxy, image.shape[:2]).to(dev)
            masks, _, _ = host_pred.predict_torch(point_coords=None, point_labels=None, boxes=prompts[:1], multimask_output=False)      # the first kept box alone
            out.append(masks[0].squeeze(0))
        return out

    def path_b():
        return g.predict_masks(image_d, ids, box_threshold=threshold)

    for _ in range(2):
        ma, mb = path_a(), path_b()
    same = [bool(torch.equal(ma[i], mb[0][i])) for i in range(2)]
    emit(f"masks of (b) equal to (a): {same}; found {mb[2].tolist()}; mask areas {[round(float(m.float().mean()), 4) for m in mb[0]]}")
    graph = bert_bench.graph_of(path_b)
    r = rounds([path_a, path_b, graph.replay], a.calls)
    for i, x in enumerate(r):
        emit(f"round {i + 1}: (a) host path, the two captions one after the other {x[0]:.2f} ms; (b) predict_masks eager {x[1]:.2f} ms; (c) predict_masks from a graph {x[2]:.2f} ms")
    ok_b, ok_c = all(x[1] <= x[0] for x in r), all(x[2] <= x[0] for x in r)
    emit(f"(b) is {'not slower' if ok_b else 'SLOWER'} than (a) in both rounds; (c) is {'not slower' if ok_c else 'SLOWER'} than (a) in both rounds")

    lut = image_prep.lut_unit_mean_std(gs.MEAN, gs.STD, dt, dev)

    def dev_resize():
        return ops.image_prep(image_d, (800, 800), image_prep.BILINEAR, lut=lut)

    for _ in range(2):
        xh, xd = host_input(), dev_resize()
    emit(f"(d) the device result equals the host's: {bool(torch.equal(xh, xd))}")
    gr = bert_bench.graph_of(dev_resize)
    rd = rounds([host_input, dev_resize, gr.replay], 4 * a.calls)
    for i, x in enumerate(rd):
        emit(f"round {i + 1}: (d) 1024 x 1024 -> 800 x 800 to the detector's fp16 input: PIL + normalise + upload on the host {x[0]:.3f} ms; "
             f"ops.image_prep eager {x[1]:.3f} ms; from a graph {x[2]:.3f} ms")
    ok_d = all(x[1] <= x[0] for x in rd)
    emit(f"(d) the device side is {'not slower' if ok_d else 'SLOWER'} than the host side in both rounds")
    if not (ok_b and ok_c and ok_d):
        sys.exit(1)


if __name__ == "__main__":
    main()
