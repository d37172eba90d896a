"""Golden vectors of the segmenter from an image and a prompt to a mask: the REFERENCE's own ``EfficientViTSam`` /
``EfficientViTSamPredictor`` (set_image, predict, predict_torch, postprocess_masks), on the CPU in fp32.

    python tests/golden/make_golden_sam.py        (needs /root/reference; writes sam_golden.npz next to itself)

The reference imports ``PromptEncoder`` / ``MaskDecoder`` / ``TwoWayTransformer`` from ``segment_anything`` and its image transform from
``torchvision``; neither is installed.  tests/sam_torch.py's classes stand in for the former (pinned against ``transformers`` by
tests/test_sam.py), and for the latter the few lines below that do what torchvision does to a PIL image: ``to_pil_image`` /
``resize`` (PIL, bilinear), ``ToTensor`` (HWC uint8 -> CHW float / 255), ``Normalize``, ``Compose``.

The model is narrow: the encoder of make_golden_effvit.py (same config, same seed, hence the ``sd.*`` of effvit_golden.npz, asserted
here), 128 x 128 encoder input, prompts in a 256 frame (``image_size = (256, 128)``), a decoder with ``mlp_dim`` 128.  SAM's width of 256
is fixed by the encoder's LayerNorm2d, so the decoder still has 1.5 M parameters, more than a committed fixture may hold: the file keeps
the prompt encoder's tensors, and for the decoder the seed of ``sam_torch.seed_state`` with a checksum per key.

Two images.  ``image`` is 96 x 128: its long side already is the encoder's 128, so pad, crop and the final resize act
(input_size 192 x 256 -> 96 x 128); everything below is recorded for it.  ``image_b`` is 60 x 100: the PIL resize acts too
(77 x 128); its resized uint8 image, encoder input and one box's result are recorded.

What is written (maps subsampled as noted, to stay within the size of a committed fixture):
  cfg_*                         image_size, mlp_dim, seeds, subsampling strides
  sd_keys, sd_shapes_*, sum.*   every prompt_encoder.* / mask_decoder.* key, its shape and sam_torch.checksum
  sd.prompt_encoder.*           the prompt encoder's tensors (fp16 grid)
  image, image_b, resized_b     uint8
  enc_in, enc_in_b              the encoder's input [1, 3, 128, 128] at [::2, ::2]
  features                      the embedding at [::8, ::8]
  boxes, boxes_in, points, point_labels, points_in      prompts in the image's pixels and after apply_boxes / apply_coords
  sparse_boxes, sparse_points, dense, dense_pe          prompt encoder outputs (dense_pe at [::8, ::8])
  layer{i}_queries, layer{i}_keys, final_queries        the two-way transformer per layer for the three boxes (keys at pixels [::16, ::16])
  low_boxes, iou_boxes          predict_torch(boxes, multimask_output=False): logits at [::4, ::4], IoU
  low_multi, iou_multi          the same for box 0 with multimask_output=True
  logits_boxes, masks_boxes     final logits and masks [3, 1, 96, 128]
  low_points, iou_points, masks_points    predict(point_coords, point_labels) with multimask_output=True
  masks_box_predict             predict(box=boxes[0], multimask_output=False)[0]
  masks_b, logits_b, low_b      image_b, one box (low_b at [::4, ::4])
  excluded_share, twin_low_err  the share of final logits within MASK_MULT x the fp16 twin's low-resolution logit error of the threshold; asserted <= 1 %
"""
import copy
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden_effvit as ge          # noqa: E402
import sam_torch as st                   # noqa: E402

IMAGE_SIZE = (256, 128)
MLP_DIM = 128
SEED_ENC, SEED_PE, SEED_MD, SEED_IMG = 20, 31, 56, 33
SUB_EMB, SUB_LOW, SUB_KEYS = 8, 4, 16
# the test compares masks where |golden logit| exceeds MASK_MULT x (measured low-resolution logit error); for "is the seed good" that
# error is measured here on an fp16 twin of the model (see main)
MASK_MULT = 2.0


def install_transform_stand_ins():
    from PIL import Image
    tv = sys.modules["torchvision.transforms"]
    tf = sys.modules["torchvision.transforms.functional"]

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class ToTensor:
        def __call__(self, a):
            return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).float().div(255)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = torch.tensor(mean)[:, None, None], torch.tensor(std)[:, None, None]

        def __call__(self, x):
            return (x - self.mean) / self.std

    tv.Compose, tv.ToTensor, tv.Normalize = Compose, ToTensor, Normalize
    tf.to_pil_image = lambda a: Image.fromarray(np.ascontiguousarray(a))
    tf.resize = lambda img, size: img.resize((size[1], size[0]), Image.BILINEAR)

    class ResizeLongestSide:
        get_preprocess_shape = staticmethod(st.get_preprocess_shape)

    sys.modules["segment_anything.utils.transforms"].ResizeLongestSide = ResizeLongestSide
    for name in ("segment_anything.modeling", "segment_anything.modeling.mask_decoder", "segment_anything.modeling.prompt_encoder"):
        m = sys.modules[name]
        m.MaskDecoder, m.PromptEncoder, m.TwoWayTransformer = st.MaskDecoder, st.PromptEncoder, st.TwoWayTransformer


ROUND = lambda m_, i_, o_: o_.half().float() if torch.is_tensor(o_) else o_


def half_decoder(pred, boxes):
    """predict_torch's low-resolution logits with every activation of the decoder rounded to fp16 where the HIP path stores one:
    after each Linear, LayerNorm, attention and upscaling layer (forward hooks), on features of the fp16 encoder."""
    md = pred.model.mask_decoder
    hooks = [m.register_forward_hook(ROUND) for m in md.modules() if isinstance(m, (torch.nn.Linear, torch.nn.LayerNorm, torch.nn.ConvTranspose2d, torch.nn.GELU, st.LayerNorm2d))]
    low = pred.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)[2]
    for h in hooks:
        h.remove()
    return low


def main():
    ge.install_stand_ins()
    install_transform_stand_ins()
    backbone, sam = ge.import_reference()
    c = ge.NARROW
    bb = backbone.EfficientViTLargeBackbone(width_list=c["width_list"], depth_list=c["depth_list"], qkv_dim=c["qkv_dim"])
    neck = sam.SamNeck(fid_list=c["neck_fids"], in_channel_list=[c["width_list"][int(f[-1])] for f in c["neck_fids"]],
                       head_width=c["head_width"], head_depth=c["head_depth"], expand_ratio=c["neck_expand"], middle_op=c["neck_middle"])
    enc = sam.EfficientViTSamImageEncoder(bb, neck).eval()
    ge.seed_model(enc, SEED_ENC)
    eff = np.load(os.path.join(HERE, "effvit_golden.npz"))
    for k, v in enc.state_dict().items():
        assert np.array_equal(eff["sd." + k], v.numpy()), f"encoder key {k} differs from effvit_golden.npz"
    pe, md = st.build((64, 64), (IMAGE_SIZE[0], IMAGE_SIZE[0]), mlp_dim=MLP_DIM)
    st.seed_state(pe, SEED_PE)
    st.seed_state(md, SEED_MD)
    model = sam.EfficientViTSam(enc, pe, md, image_size=IMAGE_SIZE).eval()
    pred = sam.EfficientViTSamPredictor(model)

    rs = np.random.RandomState(SEED_IMG)
    smooth = lambda h, w: np.clip(np.kron(rs.randint(0, 256, (h // 4 + 1, w // 4 + 1, 3)), np.ones((4, 4, 1)))[:h, :w] + rs.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    image, image_b = smooth(96, 128), smooth(60, 100)
    out = {"cfg_image_size": np.array(IMAGE_SIZE), "cfg_mlp_dim": np.array(MLP_DIM), "cfg_seed_pe": np.array(SEED_PE), "cfg_seed_md": np.array(SEED_MD),
           "cfg_sub_emb": np.array(SUB_EMB), "cfg_sub_low": np.array(SUB_LOW), "cfg_sub_keys": np.array(SUB_KEYS), "cfg_mask_mult": np.array(MASK_MULT), "image": image, "image_b": image_b}
    keys = []
    for prefix, mod in (("prompt_encoder", pe), ("mask_decoder", md)):
        for k, v in mod.state_dict().items():
            keys.append(f"{prefix}.{k}")
            out[f"sum.{prefix}.{k}"] = st.checksum(v)
            out[f"shape.{prefix}.{k}"] = np.array(v.shape, dtype=np.int64)
            if prefix == "prompt_encoder":
                out[f"sd.{prefix}.{k}"] = v.numpy()
    out["sd_keys"] = np.array(keys)

    with torch.no_grad():
        # ---- image: 96 x 128
        pred.set_image(image)
        assert pred.input_size == (192, 256) and tuple(pred.original_size) == (96, 128)
        enc_in = model.transform(image).unsqueeze(0)
        assert enc_in.shape == (1, 3, 128, 128)
        out["enc_in"] = enc_in[:, :, ::2, ::2].contiguous().numpy()
        out["features"] = pred.features[:, :, ::SUB_EMB, ::SUB_EMB].contiguous().numpy()
        boxes = np.array([[10.0, 8.0, 70.0, 60.0], [40.5, 30.25, 120.0, 90.0], [0.0, 0.0, 127.0, 95.0]])
        points, labels = np.array([[30.0, 40.0], [100.5, 20.0], [64.0, 80.0]]), np.array([1, 0, 1])
        out["boxes"], out["points"], out["point_labels"] = boxes, points, labels.astype(np.int64)
        out["boxes_in"], out["points_in"] = pred.apply_boxes(boxes), pred.apply_coords(points)
        bt = torch.as_tensor(out["boxes_in"], dtype=torch.float)
        sparse, dense = pe(points=None, boxes=bt, masks=None)
        out["sparse_boxes"], out["dense"] = sparse.numpy(), dense[0, :, 0, 0].contiguous().numpy()
        pt = (torch.as_tensor(out["points_in"], dtype=torch.float)[None], torch.as_tensor(labels, dtype=torch.int)[None])
        out["sparse_points"] = pe(points=pt, boxes=None, masks=None)[0].numpy()
        out["dense_pe"] = pe.get_dense_pe()[:, :, ::SUB_EMB, ::SUB_EMB].contiguous().numpy()

        md.transformer.trace = []
        masks, iou, low = pred.predict_torch(point_coords=None, point_labels=None, boxes=bt, multimask_output=False)
        logits = pred.predict_torch(point_coords=None, point_labels=None, boxes=bt, multimask_output=False, return_logits=True)[0]
        trace, md.transformer.trace = md.transformer.trace[:3], None
        for i, (q, k) in enumerate(trace[:2]):
            out[f"layer{i}_queries"] = q.numpy()
            out[f"layer{i}_keys"] = k.reshape(3, 64, 64, 256)[:, ::SUB_KEYS, ::SUB_KEYS].contiguous().numpy()
        out["final_queries"] = trace[2][0].numpy()
        assert masks.shape == (3, 1, 96, 128) and masks.dtype == torch.bool and low.shape == (3, 1, 256, 256) and iou.shape == (3, 1)
        assert torch.equal(masks, logits > 0)
        out["low_boxes"], out["iou_boxes"] = low[:, :, ::SUB_LOW, ::SUB_LOW].contiguous().numpy(), iou.numpy()
        out["low_rms"] = np.array(float(low.pow(2).mean().sqrt()))
        out["logits_boxes"], out["masks_boxes"] = logits.numpy(), masks.numpy()
        _, iou_m, low_m = pred.predict_torch(point_coords=None, point_labels=None, boxes=bt[:1], multimask_output=True)
        out["low_multi"], out["iou_multi"] = low_m[:, :, ::SUB_LOW, ::SUB_LOW].contiguous().numpy(), iou_m.numpy()
        m1, i1, l1 = pred.predict(box=boxes[0], multimask_output=False)
        assert m1.shape == (1, 96, 128) and i1.shape == (1,) and l1.shape == (1, 256, 256) and np.array_equal(m1, masks[0].numpy())
        out["masks_box_predict"] = m1
        mp, ip, lp = pred.predict(point_coords=points, point_labels=labels, multimask_output=True)
        assert mp.shape == (3, 96, 128)
        out["masks_points"], out["iou_points"], out["low_points"] = mp, ip, np.ascontiguousarray(lp[:, ::SUB_LOW, ::SUB_LOW])

        # the storage-dtype twin: the same model with every layer's output rounded to fp16; its low-resolution logit error stands for the one the
        # test will measure, and the share of pixels within MASK_MULT x that error of the threshold must leave room below 2 %
        twin = sam.EfficientViTSamPredictor(copy.deepcopy(model))
        twin.is_image_set, twin.original_size, twin.input_size = True, pred.original_size, pred.input_size
        hooks = [m.register_forward_hook(ROUND) for m in twin.model.image_encoder.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.BatchNorm2d))]
        twin.features = twin.model.image_encoder(enc_in.half().float()).half().float()
        for h in hooks:
            h.remove()
        low16 = half_decoder(twin, bt)
        err = float((low16 - low).abs().max())
        share = float(np.mean(np.abs(out["logits_boxes"]) <= MASK_MULT * err))
        out["excluded_share"], out["twin_low_err"] = np.array(share), np.array(err)
        print(f"fp16 twin: low-resolution logit error {err:.3e} (rms {float(out['low_rms']):.3e}); excluded share at {MASK_MULT} x that: {share:.4f}")
        print("per box: mask area", out["masks_boxes"].mean(axis=(1, 2, 3)), "share", [float(np.mean(np.abs(l) <= MASK_MULT * err)) for l in out["logits_boxes"]])
        assert share <= 0.01, share

        # ---- image_b: 60 x 100, resized to 77 x 128
        pred.set_image(image_b)
        assert pred.input_size == (154, 256)
        out["resized_b"] = sam.SamResize(IMAGE_SIZE[1])(image_b)
        assert out["resized_b"].shape == (77, 128, 3) and out["resized_b"].dtype == np.uint8
        out["enc_in_b"] = model.transform(image_b).unsqueeze(0)[:, :, ::2, ::2].contiguous().numpy()
        box_b = np.array([12.0, 9.0, 80.0, 50.0])
        out["box_b"] = box_b
        out["masks_b"], _, low_b = pred.predict(box=box_b, multimask_output=False)
        out["low_b"] = np.ascontiguousarray(low_b[:, ::SUB_LOW, ::SUB_LOW])
        out["logits_b"] = pred.predict(box=box_b, multimask_output=False, return_logits=True)[0]
    path = os.path.join(HERE, "sam_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("sam_golden.npz:", len(out), "arrays,", size, "bytes; mask areas", out["masks_boxes"].mean(axis=(1, 2, 3)), "iou", out["iou_boxes"].ravel())
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
