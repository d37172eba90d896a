#!/usr/bin/env python
"""A/B of the whole segmenter call, ``set_image`` + ``predict_torch``, at full width: efficientvit_sam("l0") (512 x 512 encoder input,
prompts in a 1024 frame) on a 1024 x 1024 image with one box and with eight, this package's modules (omg_amd/sam.py) against the same
modules evaluated per layer by torch on the GPU in fp16 (the encoder as tests/effvit_torch.py's TorchEncoder, the decoder as
tests/sam_torch.py's classes moved to the device, postprocess_masks as two F.interpolate calls).  The host part of ``set_image``
(PIL resize, mean / std, pad, upload) is the same code on both sides and is inside both timings; the per-layer side encodes the
prompts on the host in fp32 (a few hundred flops) and caches the dense positional encoding, as the module does.

    python tools/sam_bench.py [--log profiles/sam_ab.log] [--boxes 1 8]

Per box count: seeded weights, 3 warm-up calls of each path, then per-layer / module interleaved, 7 synchronised calls each, the
median reported.  Nothing is promised about the ratio; the log says what was measured.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from omg_amd import sam
from tests import sam_torch as st
from tests.effvit_torch import TorchEncoder, seed_encoder


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--boxes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--calls", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = sam.efficientvit_sam("l0", device=dev)
    seed_encoder(model.image_encoder, 30)
    pe, md = st.build()
    st.seed_state(pe, 31), st.seed_state(md, 32)
    sd = {"prompt_encoder." + k: v for k, v in pe.state_dict().items()}
    sd.update({"mask_decoder." + k: v for k, v in md.state_dict().items()})
    model.load_state_dict(sd, strict=False)
    pred = sam.EfficientViTSamPredictor(model)
    fb_enc = TorchEncoder(model.image_encoder, rounded=True)
    md16 = md.half().to(dev)
    dense_pe16 = pe.get_dense_pe().half().to(dev)
    image = np.random.RandomState(0).randint(0, 256, (1024, 1024, 3)).astype(np.uint8)
    rs = np.random.RandomState(1)

    lines = [f"EfficientViT-SAM l0, set_image + predict_torch on a 1024x1024 image, fp16, {torch.cuda.get_device_name(0)}; "
             f"median of {a.calls} synchronised calls, interleaved"]
    for n in a.boxes:
        xy = rs.uniform(0, 500, (n, 2))
        boxes_np = np.concatenate([xy, xy + rs.uniform(100, 500, (n, 2))], axis=1)

        def new():
            pred.set_image(image)
            boxes = torch.as_tensor(pred.apply_boxes(boxes_np), dtype=torch.float, device=dev)
            return pred.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)

        def old():
            pred._set_sizes(image.shape[:2])
            _, x = model.preprocess(image)
            feat = fb_enc.features(x.to(dev, torch.float16))["out"]
            with torch.no_grad():
                sparse, dense = pe(points=None, boxes=torch.as_tensor(pred.apply_boxes(boxes_np), dtype=torch.float), masks=None)
                low, iou = md16(feat, dense_pe16, sparse.half().to(dev), dense[:1].half().to(dev), False)
                masks = st.postprocess_masks(low.float(), model.image_size[0], pred.input_size, pred.original_size) > model.mask_threshold
            return masks, iou, low

        for _ in range(3):
            old(); new()
        m_old, m_new = old()[0], new()[0]
        agree = (m_old == m_new).float().mean().item()
        t_old, t_new = [], []
        for _ in range(a.calls):
            t_old.append(timed(old))
            t_new.append(timed(new))
        mo, mn = statistics.median(t_old), statistics.median(t_new)
        lines.append(f"{n} box(es): per-layer torch {mo:.3f} ms  (min {min(t_old):.3f}, max {max(t_old):.3f});  "
                     f"HIP modules {mn:.3f} ms  (min {min(t_new):.3f}, max {max(t_new):.3f});  per-layer / modules = {mo / mn:.2f};  "
                     f"mask pixels equal on both paths: {100 * agree:.2f} %")
    text = "\n".join(lines)
    print(text)
    if a.log:
        with open(a.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
