"""Generate tests/golden/sam_vit_golden.npz: what SAM's ViT image encoder, the whole ``Sam`` and the predictor's flow compute in fp32.

    python tests/golden/make_golden_sam_vit.py        (from the repository root; CPU only, under a minute)

The oracle is tests/sam_vit_torch.py (pinned against ``transformers`` by tests/test_sam_vit.py); nothing outside the repository is
read.  Two narrow models at the real 64 x 64 token grid (1024 x 1024 input, 14 x 14 windows: 25 windows of which 9 are padded):

    d64   embed_dim 128 = 2 heads x 64        d80   embed_dim 320 = 4 heads x 80
    depth 4, global attention in blocks 1 and 3, mlp_ratio 4; the full-size prompt encoder; a mask decoder with mlp_dim 128

Stored, per model under the prefix ``d64.`` / ``d80.``:
  cfg_*                       the constructor arguments and the seeds (weights are regenerated: seed_vit / seed_state)
  sd_keys, sum.<key>          the state-dict keys and a float64 checksum per key
  patch_embed, block0 .. 3    NHWC activations at the token rows / columns ``cfg_idx`` (window corners, padded windows, the last token)
  features                    the embedding [1, 256, 64, 64] at the same positions
  low_* / iou_* / logits_* / masks_*   the predictor's returns for three boxes, for three points (multimask), and for image_b's box;
                              low-resolution logits at every ``cfg_sub_low``-th pixel
  twin_low_err, excluded_share   the low-resolution logit error of an fp16-rounded twin (forward hooks on every layer, as
                              make_golden_sam.py's half_decoder), and the share of final logits within MASK_MULT x that error of the
                              threshold: asserted <= 1 %, so that the mask test's 2 % cap is met by the reference alone
Shared: image_a (48 x 64, resized to 768 x 1024 through PIL), image_b (16 x 1024: no resize), the prompts in image pixels and in the
input frame, a checksum of the resized image_a."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import sam_torch as st  # noqa: E402
from tests import sam_vit_torch as vt  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sam_vit_golden.npz")
MODELS = {"d64": dict(embed_dim=128, depth=4, heads=2, mlp_dim=128, seed_enc=14, seed_pe=1, seed_md=3),
          "d80": dict(embed_dim=320, depth=4, heads=4, mlp_dim=128, seed_enc=13, seed_pe=1, seed_md=2)}
GLOBAL = (1, 3)
IDX = [0, 14, 31, 57, 63]
SUB_LOW = 8
MASK_MULT = 2.0
BOXES = np.array([[4.0, 3.0, 40.0, 30.0], [20.0, 10.0, 62.0, 46.0], [0.0, 20.0, 30.0, 47.0]])
POINTS = np.array([[12.0, 9.0], [50.0, 40.0], [33.0, 24.0]])
POINT_LABELS = np.array([1, 0, 1], dtype=np.int32)
BOX_B = np.array([100.0, 2.0, 800.0, 14.0])


def make_image(h, w, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        img[..., c] = 128 + 70 * np.sin(2 * np.pi * (x / w * (1.5 + c) + y / h * (0.7 + 0.5 * c))) + 40 * np.cos(2 * np.pi * (y / h * (2 + c) - x / w))
    for _ in range(6):
        cy, cx, r = rs.uniform(0, h), rs.uniform(0, w), rs.uniform(0.1, 0.3) * max(h, w)
        img[((y - cy) ** 2 + (x - cx) ** 2) < r * r] += rs.uniform(-90, 90, 3)
    img += rs.normal(0, 6, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


ROUND = lambda m_, i_, o_: o_.half().float() if torch.is_tensor(o_) else o_


def fp16_twin_low(sam, image, original_size, boxes_in, points=None):
    """The low-resolution logits (for the boxes; and for the points, multimask) with every layer's output rounded to fp16 where the HIP
    path stores one."""
    kinds = (torch.nn.Linear, torch.nn.LayerNorm, torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.GELU, st.LayerNorm2d, vt.MLPBlock, vt.Attention)
    hooks = [m.register_forward_hook(ROUND) for m in sam.modules() if isinstance(m, kinds)]
    feat, input_size = vt.embed(sam, image)
    low = vt.predict(sam, feat, input_size, original_size, boxes=boxes_in)[2]
    low_p = vt.predict(sam, feat, input_size, original_size, points=points, multimask=True)[2] if points is not None else None
    for h in hooks:
        h.remove()
    return low, low_p


def at(t):
    """NHWC or NCHW-by-flag subsample at IDX x IDX."""
    i = torch.tensor(IDX)
    return t[:, i][:, :, i]


def main():
    torch.manual_seed(0)
    image_a, image_b = make_image(48, 64, 1), make_image(16, 1024, 2)
    boxes_in = vt.apply_coords(BOXES.reshape(-1, 2, 2), (48, 64)).reshape(-1, 4)
    points_in = vt.apply_coords(POINTS, (48, 64))
    box_b_in = vt.apply_coords(BOX_B.reshape(-1, 2, 2), (16, 1024)).reshape(-1, 4)
    assert np.array_equal(box_b_in[0], BOX_B)
    out = {"image_a": image_a, "image_b": image_b, "boxes": BOXES, "boxes_in": boxes_in, "points": POINTS, "point_labels": POINT_LABELS, "points_in": points_in,
           "box_b": BOX_B, "cfg_idx": np.array(IDX), "cfg_sub_low": np.array(SUB_LOW), "cfg_mask_mult": np.array(MASK_MULT),
           "resized_a_sum": st.checksum(torch.from_numpy(vt.resize_longest(image_a).astype(np.float64)))}
    assert vt.resize_longest(image_a).shape == (768, 1024, 3) and vt.resize_longest(image_b) .shape == (16, 1024, 3)
    assert np.array_equal(vt.resize_longest(image_b), image_b)
    for name, c in MODELS.items():
        P = name + "."
        for k, v in c.items():
            out[P + "cfg_" + k] = np.array(v)
        out[P + "cfg_global"] = np.array(GLOBAL)
        gold_cfg = {k: v for k, v in out.items()}
        sam = vt.seeded_oracle(gold_cfg, name)
        sd = sam.state_dict()
        out[P + "sd_keys"] = np.array(list(sd))
        for k, v in sd.items():
            out[P + "sum." + k] = st.checksum(v)
        sam.image_encoder.trace = {}
        feat, input_size = vt.embed(sam, image_a)
        assert input_size == (768, 1024) and feat.shape == (1, 256, 64, 64)
        for k, v in sam.image_encoder.trace.items():
            out[P + k] = at(v).numpy()
        sam.image_encoder.trace = None
        out[P + "features"] = at(feat.permute(0, 2, 3, 1)).permute(0, 3, 1, 2).numpy()
        bt = torch.from_numpy(boxes_in).float()
        logits, iou, low = vt.predict(sam, feat, input_size, (48, 64), boxes=bt)
        assert logits.shape == (3, 1, 48, 64) and low.shape == (3, 1, 256, 256) and iou.shape == (3, 1)
        out[P + "logits_boxes"], out[P + "masks_boxes"], out[P + "iou_boxes"] = logits.numpy(), (logits > 0).numpy(), iou.numpy()
        out[P + "low_boxes"] = low[:, :, ::SUB_LOW, ::SUB_LOW].numpy()
        pts = (torch.from_numpy(points_in).float()[None], torch.from_numpy(POINT_LABELS)[None])
        lg, io, lo = vt.predict(sam, feat, input_size, (48, 64), points=pts, multimask=True)
        assert lg.shape == (1, 3, 48, 64)
        out[P + "logits_points"], out[P + "masks_points"], out[P + "iou_points"], out[P + "low_points"] = lg.numpy(), (lg > 0).numpy(), io.numpy(), lo[:, :, ::SUB_LOW, ::SUB_LOW].numpy()
        # the guard of the mask test: boxes and points, each against the fp16 twin's own error
        twin, twin_p = fp16_twin_low(sam, image_a, (48, 64), bt, pts)
        err, err_p = float((twin - low).abs().max()), float((twin_p - lo).abs().max())
        share = float(np.mean(np.abs(out[P + "logits_boxes"]) <= MASK_MULT * err))
        share_p = float(np.mean(np.abs(out[P + "logits_points"]) <= MASK_MULT * err_p))
        out[P + "twin_low_err"], out[P + "excluded_share"], out[P + "low_rms"] = np.array([err, err_p]), np.array([share, share_p]), np.array(float(low.pow(2).mean().sqrt()))
        areas = list(out[P + "masks_boxes"].mean(axis=(1, 2, 3))) + list(out[P + "masks_points"].mean(axis=(0, 2, 3)))
        print(f"{name}: fp16 twin low-resolution logit error {err:.3e} / {err_p:.3e} (rms {float(out[P + 'low_rms']):.3e}); excluded share at {MASK_MULT} x that: "
              f"{share:.4f} / {share_p:.4f}; mask areas (3 boxes, 3 point masks) {np.round(areas, 3)}")
        assert share <= 0.01 and share_p <= 0.01, (share, share_p)
        assert any(0.02 < a < 0.98 for a in areas), "every mask is (nearly) empty or full"
        # the second image: no resize, another input_size
        feat_b, input_b = vt.embed(sam, image_b)
        assert input_b == (16, 1024)
        bb = torch.from_numpy(box_b_in).float()
        lg, io, lo = vt.predict(sam, feat_b, input_b, (16, 1024), boxes=bb)
        out[P + "logits_b"], out[P + "masks_b"], out[P + "iou_b"], out[P + "low_b"] = lg.numpy(), (lg > 0).numpy(), io.numpy(), lo[:, :, ::SUB_LOW, ::SUB_LOW].numpy()
        twin_b = fp16_twin_low(sam, image_b, (16, 1024), bb)[0]
        err_b = float((twin_b - lo).abs().max())
        share_b = float(np.mean(np.abs(out[P + "logits_b"]) <= MASK_MULT * err_b))
        print(f"{name}, image_b: twin error {err_b:.3e}, excluded share {share_b:.4f}, mask area {out[P + 'masks_b'].mean():.3f}")
        assert share_b <= 0.01, share_b
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes, {len(out)} arrays")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
