"""Golden vectors of the xl segmenter from an image and a box to a mask: the REFERENCE's own ``EfficientViTSam`` /
``EfficientViTSamPredictor`` on the narrow six-stage encoder of make_golden_effvit_xl.py, on the CPU in fp32, after the reference's
``set_norm_eps(model, 1e-6)`` on the WHOLE model (what its ``create_sam_model`` does).

    python tests/golden/make_golden_sam_xl.py        (needs the reference checkout make_golden_effvit.py points to; writes sam_xl_golden.npz next to itself)

The protocol of make_golden_sam.py on a smaller scale; its stand-ins for ``segment_anything`` and ``torchvision`` are used as they are.
``image_size = (128, 128)``: both entries equal, as in the xl models (1024, 1024), so prompts, ``input_size`` and the encoder's input
share one frame.  One image, 60 x 100: its long side needs the PIL resize (77 x 128), then pad, crop and the final resize act.

What is written:
  cfg_*                         image_size, mlp_dim, seeds, eps, subsampling strides, mask_mult
  image                         uint8 [60, 100, 3]
  features                      the embedding at [::8, ::8]
  boxes, boxes_in               three boxes in the image's pixels and after apply_boxes
  low_boxes, iou_boxes, low_rms predict_torch(boxes, multimask_output=False): logits at [::4, ::4], IoU
  logits_boxes, masks_boxes     final logits and masks [3, 1, 60, 100]
  masks_box_predict             predict(box=boxes[0], multimask_output=False)[0]
  excluded_share, twin_low_err  the share of final logits within MASK_MULT x the fp16 twin's low-resolution logit error of the threshold; asserted <= 1 %
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden_effvit as ge          # noqa: E402
import make_golden_effvit_xl as gx       # noqa: E402
import make_golden_sam as gs             # noqa: E402
import sam_torch as st                   # noqa: E402

IMAGE_SIZE = (128, 128)
MLP_DIM = 128
SEED_PE, SEED_MD, SEED_IMG = 61, 362, 64          # the decoder seed was searched: few pixels near the threshold, masks not all one value
SUB_EMB, SUB_LOW = 8, 4
MASK_MULT = gs.MASK_MULT


def main():
    ge.install_stand_ins()
    gs.install_transform_stand_ins()
    backbone, sam = ge.import_reference()
    set_norm_eps = sys.modules["src.efficientvit.models.nn.norm"].set_norm_eps
    enc = gx.build_encoder(backbone, sam)
    eff = np.load(os.path.join(HERE, "effvit_xl_golden.npz"))
    for k, v in enc.state_dict().items():
        assert np.array_equal(eff["sd." + k], v.numpy()), f"encoder key {k} differs from effvit_xl_golden.npz"
    pe, md = st.build((64, 64), (IMAGE_SIZE[0], IMAGE_SIZE[0]), mlp_dim=MLP_DIM)
    st.seed_state(pe, SEED_PE)
    st.seed_state(md, SEED_MD)
    model = sam.EfficientViTSam(enc, pe, md, image_size=IMAGE_SIZE).eval()
    set_norm_eps(model, gx.EPS)
    norms = [m for m in model.modules() if isinstance(m, (torch.nn.LayerNorm, torch.nn.BatchNorm2d))]
    assert len(norms) > 10 and all(m.eps == gx.EPS for m in norms) and md.transformer.norm_final_attn.eps == gx.EPS
    assert not isinstance(md.output_upscaling[1], torch.nn.LayerNorm) and md.output_upscaling[1].eps == 1e-6      # segment_anything's LayerNorm2d: left alone
    pred = sam.EfficientViTSamPredictor(model)

    rs = np.random.RandomState(SEED_IMG)
    smooth = lambda h, w: np.clip(np.kron(rs.randint(0, 256, (h // 4 + 1, w // 4 + 1, 3)), np.ones((4, 4, 1)))[:h, :w] + rs.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    image = smooth(60, 100)
    out = {"cfg_image_size": np.array(IMAGE_SIZE), "cfg_mlp_dim": np.array(MLP_DIM), "cfg_seed_pe": np.array(SEED_PE), "cfg_seed_md": np.array(SEED_MD),
           "cfg_sub_emb": np.array(SUB_EMB), "cfg_sub_low": np.array(SUB_LOW), "cfg_mask_mult": np.array(MASK_MULT), "cfg_eps": np.array(gx.EPS), "image": image}
    with torch.no_grad():
        pred.set_image(image)
        assert pred.input_size == (77, 128) and tuple(pred.original_size) == (60, 100)
        enc_in = model.transform(image).unsqueeze(0)
        assert enc_in.shape == (1, 3, 128, 128)
        out["features"] = pred.features[:, :, ::SUB_EMB, ::SUB_EMB].contiguous().numpy()
        boxes = np.array([[8.0, 6.0, 60.0, 40.0], [30.5, 20.25, 95.0, 55.0], [0.0, 0.0, 99.0, 59.0]])
        out["boxes"], out["boxes_in"] = boxes, pred.apply_boxes(boxes)
        bt = torch.as_tensor(out["boxes_in"], dtype=torch.float)
        masks, iou, low = pred.predict_torch(point_coords=None, point_labels=None, boxes=bt, multimask_output=False)
        logits = pred.predict_torch(point_coords=None, point_labels=None, boxes=bt, multimask_output=False, return_logits=True)[0]
        assert masks.shape == (3, 1, 60, 100) and masks.dtype == torch.bool and low.shape == (3, 1, 256, 256) and iou.shape == (3, 1)
        assert torch.equal(masks, logits > 0)
        out["low_boxes"], out["iou_boxes"] = low[:, :, ::SUB_LOW, ::SUB_LOW].contiguous().numpy(), iou.numpy()
        out["low_rms"] = np.array(float(low.pow(2).mean().sqrt()))
        out["logits_boxes"], out["masks_boxes"] = logits.numpy(), masks.numpy()
        m1, i1, l1 = pred.predict(box=boxes[0], multimask_output=False)
        assert m1.shape == (1, 60, 100) and i1.shape == (1,) and l1.shape == (1, 256, 256) and np.array_equal(m1, masks[0].numpy())
        out["masks_box_predict"] = m1

        # the storage-dtype twin of make_golden_sam.py: every layer's output rounded to fp16; its low-resolution logit error stands for the
        # one the test will measure
        twin = sam.EfficientViTSamPredictor(copy.deepcopy(model))
        twin.is_image_set, twin.original_size, twin.input_size = True, pred.original_size, pred.input_size
        hooks = [m.register_forward_hook(gs.ROUND) for m in twin.model.image_encoder.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.BatchNorm2d))]
        twin.features = twin.model.image_encoder(enc_in.half().float()).half().float()
        for h in hooks:
            h.remove()
        low16 = gs.half_decoder(twin, bt)
        err = float((low16 - low).abs().max())
        share = float(np.mean(np.abs(out["logits_boxes"]) <= MASK_MULT * err))
        out["excluded_share"], out["twin_low_err"] = np.array(share), np.array(err)
        print(f"fp16 twin: low-resolution logit error {err:.3e} (rms {float(out['low_rms']):.3e}); excluded share at {MASK_MULT} x that: {share:.4f}")
        print("per box: mask area", out["masks_boxes"].mean(axis=(1, 2, 3)), "share", [float(np.mean(np.abs(l) <= MASK_MULT * err)) for l in out["logits_boxes"]])
        assert share <= 0.01, share
    path = os.path.join(HERE, "sam_xl_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("sam_xl_golden.npz:", len(out), "arrays,", size, "bytes; mask areas", out["masks_boxes"].mean(axis=(1, 2, 3)), "iou", out["iou_boxes"].ravel())
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
