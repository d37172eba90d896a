"""omg_amd — MI355X-native hot path of OMG (SDXL UNet forward, prompt-to-prompt attention
replacement, region-masked noise fusion).  See DESIGN.md."""
__version__ = "0.1.0"

_SAM = ("SamPromptEncoder", "SamMaskDecoder", "EfficientViTSam", "EfficientViTSamPredictor", "efficientvit_sam", "efficientvit_sam_xl0",
        "efficientvit_sam_xl1", "create_sam_model", "set_norm_eps", "EfficientViTSamConfig", "EfficientViTSamImageEncoder")
_SAM_VIT = ("SamImageEncoderViT",)
_SEGMENT_ANYTHING = ("Sam", "SamPredictor", "ResizeLongestSide", "build_sam", "build_sam_vit_h", "build_sam_vit_l", "build_sam_vit_b", "sam_model_registry")
_DPT = ("DPTForDepthEstimation", "DPTImageProcessor", "DPTFeatureExtractor", "depth_condition")
_SWIN = ("SwinBackbone", "swin_from_groundingdino")
_GDINO = ("GroundingDinoEncoder", "GroundingDinoEncoderOutput")
_GDINO_DECODER = ("GroundingDinoDecoderHead", "GroundingDinoDetectionOutput", "GroundingDinoDetector")
_BERT = ("BertTextEncoder",)
_CANNY = ("Canny", "canny_condition")
_GROUNDED_SAM = ("GroundedSam", "predict", "load_image_dino", "box_cxcywh_to_xyxy", "get_size_with_aspect_ratio")
__all__ = list(_SAM) + list(_SAM_VIT) + list(_SEGMENT_ANYTHING) + list(_DPT) + list(_SWIN) + list(_GDINO) + list(_GDINO_DECODER) + list(_BERT) + list(_GROUNDED_SAM) + list(_CANNY)


def __getattr__(name):          # the segmenter's public names, imported on first use (omg_amd.sam pulls in torch and the kernels' bindings)
    if name in _SAM:
        from . import sam
        return getattr(sam, name)
    if name in _SAM_VIT:
        from . import sam_vit
        return getattr(sam_vit, name)
    if name in _SEGMENT_ANYTHING:
        from . import segment_anything
        return getattr(segment_anything, name)
    if name in _DPT:
        from . import dpt
        return getattr(dpt, name)
    if name in _SWIN:
        from . import swin
        return getattr(swin, name)
    if name in _GDINO:
        from . import gdino
        return getattr(gdino, name)
    if name in _GDINO_DECODER:
        from . import gdino_decoder
        return getattr(gdino_decoder, name)
    if name in _BERT:
        from . import bert
        return getattr(bert, name)
    if name in _GROUNDED_SAM:
        from . import grounded_sam
        return getattr(grounded_sam, name)
    if name in _CANNY:
        from . import canny
        return getattr(canny, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
