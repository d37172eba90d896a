"""The reference's stage hand-off with ``--segment_type GroundingDINO``: the stage-1 image -> per concept word a region mask, with the
image on the device from the VAE's decode to the masks.

The names the reference's scripts import from the original ``groundingdino`` package, written from their known behaviour::

    from groundingdino.util.inference import predict      ->   from omg_amd.grounded_sam import predict
    from groundingdino.util import box_ops                ->   from omg_amd import grounded_sam as box_ops
    load_image_dino (inference_lora.py's own)             ->   from omg_amd.grounded_sam import load_image_dino

and :class:`GroundedSam`, which is ``predict_mask`` of those scripts for all concept words of one image in one call: both image
preparations (ops.image_prep: Pillow's resize bit for bit, normalise / pad / cast in the same launches), the Swin backbone and SAM's
image encoder run ONCE, the text encoder, GroundingDINO's encoder and head run on the n captions against the shared feature maps, the
box of a caption is picked on the device and SAM's decoder runs on the n boxes.  From ``input_ids`` on nothing synchronises with the
host, and with ``text_backbone="hip"`` the call is capturable in one ``torch.cuda.graph`` (after one uncaptured call: the resize tables
and lookup tables are uploaded then).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import image_prep, ops
from .gdino_decoder import detect, phrases, text_masks_from_input_ids

__all__ = ["get_size_with_aspect_ratio", "load_image_dino", "box_cxcywh_to_xyxy", "preprocess_caption", "predict", "GroundedSam"]

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_LUTS = {}


def get_size_with_aspect_ratio(image_size: Sequence[int], size: int = 800, max_size: Optional[int] = 1333) -> Tuple[int, int]:
    """The original package's ``RandomResize([size], max_size)`` rule: (w, h) -> (w, h) with the short side ``size``, unless the long
    side would pass ``max_size``: then the short side shrinks so that it does not."""
    w, h = int(image_size[0]), int(image_size[1])
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


def _lut(dtype: torch.dtype, device) -> torch.Tensor:
    key = (dtype, torch.device(device))
    if key not in _LUTS:
        _LUTS[key] = image_prep.lut_unit_mean_std(MEAN, STD, dtype, device)
    return _LUTS[key]


def load_image_dino(image_source, size: int = 800, max_size: int = 1333, dtype: torch.dtype = torch.float32):
    """``(image, image_transformed)`` as the reference's function: the image as an HWC uint8 array and the detector's input [3, h, w],
    resized by :func:`get_size_with_aspect_ratio` (bilinear, through PIL), ``ToTensor``, ``Normalize``.  A PIL image or a numpy array is
    prepared on the host (fp32, on the host); a cuda uint8 [H, W, 3] tensor on the device, in ``dtype``, with the same bits."""
    if isinstance(image_source, torch.Tensor):
        if not image_source.is_cuda or image_source.dtype != torch.uint8 or image_source.dim() != 3 or image_source.shape[2] != 3:
            raise L.OmgHipError(f"load_image_dino: a tensor image is a cuda uint8 [H, W, 3] tensor, got {image_source.dtype} "
                                f"{tuple(image_source.shape)} on {image_source.device}")
        image = image_source.contiguous()
        ow, oh = get_size_with_aspect_ratio((image.shape[1], image.shape[0]), size, max_size)
        return image, ops.image_prep(image, (oh, ow), image_prep.BILINEAR, lut=_lut(dtype, image.device))
    from PIL import Image
    image = np.asarray(image_source)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise L.OmgHipError(f"load_image_dino takes an RGB PIL image or a uint8 [H, W, 3] array, got {image.dtype} {image.shape}")
    ow, oh = get_size_with_aspect_ratio((image.shape[1], image.shape[0]), size, max_size)
    resized = image if (ow, oh) == (image.shape[1], image.shape[0]) else np.asarray(
        Image.fromarray(np.ascontiguousarray(image)).resize((ow, oh), Image.BILINEAR))
    x = torch.from_numpy(np.array(resized)).permute(2, 0, 1).float().div(255)
    mean, std = torch.tensor(MEAN, dtype=torch.float32)[:, None, None], torch.tensor(STD, dtype=torch.float32)[:, None, None]
    return image, (x - mean) / std


def box_cxcywh_to_xyxy(x: torch.Tensor) -> torch.Tensor:
    x_c, y_c, w, h = x.unbind(-1)
    return torch.stack([(x_c - 0.5 * w), (y_c - 0.5 * h), (x_c + 0.5 * w), (y_c + 0.5 * h)], dim=-1)


def preprocess_caption(caption: str) -> str:
    result = caption.lower().strip()
    return result if result.endswith(".") else result + "."


def _tokenize(tokenizer, captions: List[str], device):
    if tokenizer is None:
        raise L.OmgHipError("captions as text need a tokenizer (GroundedSam(..., tokenizer=...)); or pass input_ids")
    tok = tokenizer(captions, padding="longest", return_tensors="pt")
    ids = torch.as_tensor(tok["input_ids"]).to(device=device, dtype=torch.long)
    get = lambda k: torch.as_tensor(tok[k]).to(device=device, dtype=torch.long) if k in tok and tok[k] is not None else None
    return ids, get("token_type_ids"), get("attention_mask")


def predict(model, image: torch.Tensor, caption: str, box_threshold: float, text_threshold: float, tokenizer=None, device: str = "cuda"):
    """The original package's ``predict``: ``model`` a :class:`omg_amd.GroundingDinoDetector`, ``image`` the [3, h, w] tensor of
    :func:`load_image_dino` -> (boxes [K, 4] cxcywh normalised, scores [K], phrases) on the host, the '.' removed from the phrases.  The
    tokenizer is the caller's object (``model.tokenizer`` if not given): ``tokenizer(texts, padding=..., return_tensors="pt")`` and
    ``tokenizer.decode(ids)``."""
    tokenizer = tokenizer if tokenizer is not None else getattr(model, "tokenizer", None)
    ids, types, mask = _tokenize(tokenizer, [preprocess_caption(caption)], device)
    dt = getattr(getattr(model, "head", None), "dtype", image.dtype)
    out = model(image[None].to(device=device, dtype=dt), ids, types, mask)
    boxes, scores, token_masks = detect(out, box_threshold, text_threshold)[0]
    found = [p.replace(".", "") for p in phrases(token_masks, ids[0].cpu(), tokenizer)]
    return boxes.cpu(), scores.cpu(), found


class GroundedSam:
    """``GroundedSam(detector, sam_predictor, tokenizer=None, size=800, max_size=1333)``: a :class:`omg_amd.GroundingDinoDetector` and a
    :class:`omg_amd.SamPredictor` (or ``EfficientViTSamPredictor``), both on the device."""

    def __init__(self, detector, sam_predictor, tokenizer=None, size: int = 800, max_size: int = 1333):
        self.detector, self.sam, self.tokenizer, self.size, self.max_size = detector, sam_predictor, tokenizer, int(size), int(max_size)

    @property
    def device(self):
        return self.sam.device

    def _image(self, image) -> torch.Tensor:
        if isinstance(image, torch.Tensor):
            if not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
                raise L.OmgHipError(f"GroundedSam: a tensor image is a cuda uint8 [H, W, 3] tensor, got {image.dtype} {tuple(image.shape)} "
                                    f"on {image.device}")
            return image.contiguous()
        a = np.asarray(image)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise L.OmgHipError(f"GroundedSam takes an RGB PIL image, a uint8 [H, W, 3] array or a cuda uint8 tensor, got {a.dtype} {a.shape}")
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    @torch.no_grad()
    def predict_masks(self, image, captions, box_threshold: float = 0.3, text_threshold: float = 0.25,
                      attention_mask: Optional[torch.Tensor] = None, token_type_ids: Optional[torch.Tensor] = None):
        """``captions``: a string, a list of n strings (normalised as :func:`predict` does and tokenised together, padded to the
        longest) or ``input_ids`` [n, T] on the device (``attention_mask`` defaults to ``input_ids != 0``, BERT's pad id) ->
        ``(masks [n, H, W] bool, boxes_xyxy [n, 4] in image pixels, found [n] bool)`` on the device.  A caption's box is the first
        query, in query order, whose ``sigmoid(logits).max(-1)`` is above ``box_threshold`` (the box whose mask the reference keeps);
        where no query passes, ``found`` is False and query 0 is used so that shapes do not depend on the data.  ``text_threshold``
        selects phrases only (:func:`predict`) and does not enter a mask."""
        det, sam = self.detector, self.sam
        image = self._image(image)
        dev = image.device
        if isinstance(captions, torch.Tensor):
            ids = captions.to(device=dev, dtype=torch.long)
            if ids.dim() != 2:
                raise L.OmgHipError(f"GroundedSam.predict_masks: input_ids are [n, T], got {tuple(ids.shape)}")
        else:
            texts = [captions] if isinstance(captions, str) else list(captions)
            ids, types, mask = _tokenize(self.tokenizer, [preprocess_caption(c) for c in texts], dev)
            token_type_ids = types if token_type_ids is None else token_type_ids
            attention_mask = mask if attention_mask is None else attention_mask
        n = ids.shape[0]
        token_mask = (ids != 0) if attention_mask is None else attention_mask.to(dev).bool()
        types = torch.zeros_like(ids) if token_type_ids is None else token_type_ids.to(dev)
        H, W = int(image.shape[0]), int(image.shape[1])

        # ---- the image, once: the detector's input and the backbone; SAM's input and image encoder
        _, pixel_values = load_image_dino(image, self.size, self.max_size, dtype=det.head.dtype)
        fms = det.backbone(pixel_values[None])
        fms = fms.feature_maps if hasattr(fms, "feature_maps") else fms
        sam.set_image(image)

        # ---- the n captions against the shared feature maps
        self_mask, position_ids = text_masks_from_input_ids(ids)
        text = det.text_backbone(ids, self_mask, types, position_ids)
        enc = det.encoder([f.expand(n, -1, -1, -1) for f in fms], None, text, token_mask, self_mask, position_ids)
        out = det.head(enc, token_mask)

        # ---- per caption the first query above the threshold: a masked index minimum (no argmax over ties)
        scores = out.logits.sigmoid().max(-1)[0]                                   # [n, Q]
        Q = scores.shape[1]
        index = torch.arange(Q, device=dev)[None].expand(n, -1)
        first = torch.where(scores > box_threshold, index, torch.full_like(index, Q)).min(-1)[0]
        found = first < Q
        first = torch.where(found, first, torch.zeros_like(first))
        boxes = torch.gather(out.pred_boxes, 1, first[:, None, None].expand(-1, 1, 4))[:, 0]
        x0, y0, x1, y1 = box_cxcywh_to_xyxy(boxes).unbind(-1)
        boxes_xyxy = torch.stack([x0 * W, y0 * H, x1 * W, y1 * H], dim=-1)          # * torch.Tensor([W, H, W, H]) without an upload
        prompts = sam.transform.apply_boxes_torch(boxes_xyxy, (H, W))
        masks, _, _ = sam.predict_torch(point_coords=None, point_labels=None, boxes=prompts, multimask_output=False)
        return masks[:, 0], boxes_xyxy, found

    def predict_mask(self, image, caption: str, box_threshold: float = 0.3, text_threshold: float = 0.25) -> Optional[torch.Tensor]:
        """The reference's ``predict_mask(segmentmodel, sam, image, TEXT_PROMPT, 'GroundingDINO')``: one [H, W] bool mask, or None where
        no box passes (the reference raises there, on ``masks[0]`` of nothing)."""
        masks, _, found = self.predict_masks(image, [caption], box_threshold, text_threshold)
        return masks[0] if bool(found[0]) else None
