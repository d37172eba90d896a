"""The names the reference's scripts import from ``segment_anything``, on the HIP kernels.

``inference_lora.py`` / ``inference_instantid.py --segment_type GroundingDINO`` build the original SAM::

    from segment_anything import build_sam, SamPredictor        ->   from omg_amd.segment_anything import build_sam, SamPredictor
    sam = build_sam(checkpoint=sam_checkpoint); sam.cuda(); sam = SamPredictor(sam)
    sam.set_image(image_source)
    boxes = sam.transform.apply_boxes_torch(boxes_xyxy, image_source.shape[:2])
    masks, _, _ = sam.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)

``Sam`` = the ViT image encoder (omg_amd/sam_vit.py) + ``SamPromptEncoder`` + ``SamMaskDecoder`` (omg_amd/sam.py, unchanged) under the
checkpoint's own ``image_encoder.*`` / ``prompt_encoder.*`` / ``mask_decoder.*`` keys; ``postprocess_masks`` is omg_sam_postprocess.
The resize of ``set_image`` goes through PIL on the uint8 image, as ``ResizeLongestSide.apply_image`` does; a cuda uint8 image takes
the same resize on the device (omg_amd/image_prep.py), fused with ``Sam.preprocess``.  A mask prompt is refused,
as everywhere in omg_amd; ``SamAutomaticMaskGenerator`` is not built.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import image_prep, ops
from .sam import SamMaskDecoder, SamPromptEncoder
from .sam_vit import SamImageEncoderViT

__all__ = ["Sam", "SamPredictor", "ResizeLongestSide", "build_sam", "build_sam_vit_h", "build_sam_vit_l", "build_sam_vit_b", "sam_model_registry"]


def _device_image(image: torch.Tensor, who: str) -> torch.Tensor:
    if not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise L.OmgHipError(f"{who}: a tensor image is a cuda uint8 [H, W, 3] tensor, got {image.dtype} {tuple(image.shape)} on {image.device}")
    return image.contiguous()


class ResizeLongestSide:
    """Resizes images so that the longest side is ``target_length``, and maps coordinates and boxes into the resized frame."""

    def __init__(self, target_length: int) -> None:
        self.target_length = target_length

    @staticmethod
    def get_preprocess_shape(oldh: int, oldw: int, long_side_length: int) -> Tuple[int, int]:
        scale = long_side_length * 1.0 / max(oldh, oldw)
        return int(oldh * scale + 0.5), int(oldw * scale + 0.5)

    def apply_image(self, image):
        """HWC uint8 -> HWC uint8, bilinear through PIL (as torchvision resizes a PIL image).  A cuda uint8 tensor stays on the device:
        the same resize, bit for bit, by ops.image_prep."""
        th, tw = self.get_preprocess_shape(image.shape[0], image.shape[1], self.target_length)
        if isinstance(image, torch.Tensor):
            return ops.image_prep(_device_image(image, "ResizeLongestSide.apply_image"), (th, tw), image_prep.BILINEAR)
        from PIL import Image
        return np.array(Image.fromarray(np.ascontiguousarray(image)).resize((tw, th), Image.BILINEAR))

    def apply_coords(self, coords: np.ndarray, original_size: Tuple[int, ...]) -> np.ndarray:
        old_h, old_w = original_size
        new_h, new_w = self.get_preprocess_shape(old_h, old_w, self.target_length)
        coords = np.array(coords, dtype=float, copy=True)
        coords[..., 0] = coords[..., 0] * (new_w / old_w)
        coords[..., 1] = coords[..., 1] * (new_h / old_h)
        return coords

    def apply_boxes(self, boxes: np.ndarray, original_size: Tuple[int, ...]) -> np.ndarray:
        return self.apply_coords(np.asarray(boxes).reshape(-1, 2, 2), original_size).reshape(-1, 4)

    def apply_image_torch(self, image: torch.Tensor) -> torch.Tensor:
        """BCHW float -> BCHW float (antialiased bilinear: close to, not equal to, :meth:`apply_image`)."""
        th, tw = self.get_preprocess_shape(image.shape[2], image.shape[3], self.target_length)
        return torch.nn.functional.interpolate(image, (th, tw), mode="bilinear", align_corners=False, antialias=True)

    def apply_coords_torch(self, coords: torch.Tensor, original_size: Tuple[int, ...]) -> torch.Tensor:
        old_h, old_w = original_size
        new_h, new_w = self.get_preprocess_shape(old_h, old_w, self.target_length)
        coords = coords.clone().to(torch.float)
        coords[..., 0] = coords[..., 0] * (new_w / old_w)
        coords[..., 1] = coords[..., 1] * (new_h / old_h)
        return coords

    def apply_boxes_torch(self, boxes: torch.Tensor, original_size: Tuple[int, ...]) -> torch.Tensor:
        return self.apply_coords_torch(boxes.reshape(-1, 2, 2), original_size).reshape(-1, 4)


class Sam(nn.Module):
    mask_threshold: float = 0.0
    image_format: str = "RGB"

    def __init__(self, image_encoder: SamImageEncoderViT, prompt_encoder: SamPromptEncoder, mask_decoder: SamMaskDecoder,
                 pixel_mean=(123.675, 116.28, 103.53), pixel_std=(58.395, 57.12, 57.375)) -> None:
        super().__init__()
        self.image_encoder, self.prompt_encoder, self.mask_decoder = image_encoder, prompt_encoder, mask_decoder
        dev = image_encoder.pos_embed.device
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32, device=dev).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32, device=dev).view(-1, 1, 1), False)

    @property
    def device(self):
        return self.pixel_mean.device

    @property
    def dtype(self):
        return self.image_encoder.dtype

    def preprocess(self, x: torch.Tensor) -> torch.Tensor:
        """[..., 3, h, w] in 0..255 -> fp32 (x - pixel_mean) / pixel_std, zero padded at the right and bottom to the encoder's square."""
        x = (x.float() - self.pixel_mean.float()) / self.pixel_std.float()
        side = self.image_encoder.img_size
        h, w = x.shape[-2:]
        return torch.nn.functional.pad(x, (0, side - w, 0, side - h))

    def postprocess_masks(self, masks: torch.Tensor, input_size: Tuple[int, ...], original_size: Tuple[int, ...],
                          threshold: Optional[float] = None) -> torch.Tensor:
        """fp32 low-resolution logits [B, M, h, w] -> fp32 logits at ``original_size`` (or uint8 0 / 1 against ``threshold``)."""
        return ops.sam_postprocess(masks.contiguous(), self.image_encoder.img_size, input_size, original_size, threshold=threshold)


class SamPredictor:
    def __init__(self, sam_model: Sam) -> None:
        self.model = sam_model
        self.transform = ResizeLongestSide(sam_model.image_encoder.img_size)
        self.reset_image()

    @property
    def device(self):
        return self.model.device

    def reset_image(self) -> None:
        self.is_image_set = False
        self.features = None                 # NCHW [1, 256, 64, 64], a view of the encoder's NHWC result
        self._features_nhwc = None
        self.original_size = None
        self.input_size = None

    def _lut(self) -> torch.Tensor:
        """Sam.preprocess as a [3, 256] table of the encoder's dtype (image_prep.lut_sam), built once."""
        m = self.model
        key = (m.dtype, m.device)
        if getattr(self, "_lut_key", None) != key:
            self._lut_key, self._lut_t = key, image_prep.lut_sam(m.pixel_mean, m.pixel_std, m.dtype)
        return self._lut_t

    def set_image(self, image, image_format: str = "RGB") -> None:
        """``image``: HWC uint8, a numpy array (resized through PIL on the host, as the original) or a cuda tensor: then the resize,
        Sam.preprocess, the pad and the cast are two launches of ops.image_prep on the device, with the same bits."""
        assert image_format in ["RGB", "BGR"], f"image_format must be in ['RGB', 'BGR'], is {image_format}."
        if self.device.type != "cuda":
            raise L.OmgHipError("SamPredictor needs its model on the MI355X (cuda/hip device); there is no CPU fallback")
        if isinstance(image, torch.Tensor):
            image = _device_image(image, "SamPredictor.set_image")
            if image_format != self.model.image_format:
                image = image.flip(-1).contiguous()
            side = self.model.image_encoder.img_size
            h, w = int(image.shape[0]), int(image.shape[1])
            th, tw = self.transform.get_preprocess_shape(h, w, side)
            x = ops.image_prep(image, (th, tw), image_prep.BILINEAR, lut=self._lut(), pad_hw=(side, side))[None]
            self._set_encoder_input(x, (h, w), (th, tw))
            return
        if image_format != self.model.image_format:
            image = image[..., ::-1]
        resized = self.transform.apply_image(image)
        x = torch.as_tensor(np.ascontiguousarray(resized), device=self.device).permute(2, 0, 1).contiguous()[None, :, :, :]
        self.set_torch_image(x, image.shape[:2])

    @torch.no_grad()
    def set_torch_image(self, transformed_image: torch.Tensor, original_image_size: Tuple[int, ...]) -> None:
        side = self.model.image_encoder.img_size
        assert (len(transformed_image.shape) == 4 and transformed_image.shape[1] == 3 and max(*transformed_image.shape[2:]) == side
                ), f"set_torch_image input must be BCHW with long side {side}."
        if self.device.type != "cuda" or not transformed_image.is_cuda:
            raise L.OmgHipError("SamPredictor needs its model and image on the MI355X (cuda/hip device); there is no CPU fallback")
        x = self.model.preprocess(transformed_image).to(self.model.dtype)
        self._set_encoder_input(x, original_image_size, transformed_image.shape[-2:])

    @torch.no_grad()
    def _set_encoder_input(self, x: torch.Tensor, original_image_size, input_size) -> None:
        self.reset_image()
        self.original_size = (int(original_image_size[0]), int(original_image_size[1]))
        self.input_size = tuple(int(v) for v in input_size)
        self._features_nhwc = self.model.image_encoder.forward_features(x)["out"]
        self.features = self._features_nhwc.permute(0, 3, 1, 2)
        self.is_image_set = True

    def get_image_embedding(self) -> torch.Tensor:
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) to generate an embedding.")
        return self.features

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output: bool = True, return_logits: bool = False):
        """Prompts in the original image's pixels -> (masks [C, H, W] bool or fp32 logits, IoU predictions [C], low-resolution logits
        [C, 256, 256]) as numpy arrays."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        if mask_input is not None:
            raise L.OmgHipError("SamPredictor: a mask prompt is not built; pass mask_input=None")
        device = self.device
        coords_torch = labels_torch = box_torch = None
        if point_coords is not None:
            assert point_labels is not None, "point_labels must be supplied if point_coords is supplied."
            coords_torch = torch.as_tensor(self.transform.apply_coords(point_coords, self.original_size), dtype=torch.float, device=device)[None, :, :]
            labels_torch = torch.as_tensor(point_labels, dtype=torch.int, device=device)[None, :]
        if box is not None:
            box_torch = torch.as_tensor(self.transform.apply_boxes(box, self.original_size), dtype=torch.float, device=device)[None, :]
        masks, iou, low = self.predict_torch(coords_torch, labels_torch, box_torch, None, multimask_output, return_logits=return_logits)
        return masks[0].cpu().numpy(), iou[0].cpu().numpy(), low[0].cpu().numpy()

    @torch.no_grad()
    def predict_torch(self, point_coords=None, point_labels=None, boxes=None, mask_input=None, multimask_output: bool = True,
                      return_logits: bool = False):
        """Batched prompts already in the input frame (``transform.apply_coords_torch`` / ``apply_boxes_torch``) -> (masks [B, C, H, W]
        bool or fp32 logits, IoU predictions [B, C], low-resolution logits [B, C, 256, 256]) on the device."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        if mask_input is not None:
            raise L.OmgHipError("SamPredictor: a mask prompt is not built; pass mask_input=None")
        m = self.model
        points = (point_coords, point_labels) if point_coords is not None else None
        if boxes is not None and boxes.dim() == 3:
            boxes = boxes.reshape(boxes.shape[0], -1)
        sparse, dense = m.prompt_encoder(points=points, boxes=boxes, masks=None)
        low, iou = m.mask_decoder(self._features_nhwc, m.prompt_encoder.get_dense_pe(), sparse, dense, multimask_output)
        if return_logits:
            masks = m.postprocess_masks(low, self.input_size, self.original_size)
        else:
            masks = m.postprocess_masks(low, self.input_size, self.original_size, threshold=m.mask_threshold).bool()
        return masks, iou, low


def _build_sam(embed_dim, depth, num_heads, global_attn_indexes, checkpoint=None, dtype=torch.float16, device=None) -> Sam:
    sam = Sam(SamImageEncoderViT(img_size=1024, patch_size=16, in_chans=3, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4.0,
                                 out_chans=256, window_size=14, global_attn_indexes=global_attn_indexes, dtype=dtype, device=device),
              SamPromptEncoder(256, (64, 64), (1024, 1024), 16, dtype=dtype, device=device),
              SamMaskDecoder(256, 3, 2, 8, 2048, 3, 256, dtype=dtype, device=device))
    if checkpoint is not None:
        with open(checkpoint, "rb") as f:
            sd = torch.load(f, map_location="cpu")
        own = sam.state_dict()
        sam.load_state_dict({k: (v.to(own[k].dtype) if k in own and v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    return sam


def build_sam_vit_h(checkpoint=None, dtype=torch.float16, device=None) -> Sam:
    return _build_sam(1280, 32, 16, (7, 15, 23, 31), checkpoint, dtype, device)


def build_sam_vit_l(checkpoint=None, dtype=torch.float16, device=None) -> Sam:
    return _build_sam(1024, 24, 16, (5, 11, 17, 23), checkpoint, dtype, device)


def build_sam_vit_b(checkpoint=None, dtype=torch.float16, device=None) -> Sam:
    return _build_sam(768, 12, 12, (2, 5, 8, 11), checkpoint, dtype, device)


build_sam = build_sam_vit_h

sam_model_registry = {"default": build_sam_vit_h, "vit_h": build_sam_vit_h, "vit_l": build_sam_vit_l, "vit_b": build_sam_vit_b}
