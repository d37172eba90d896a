"""omg_amd — MI355X-native hot path of OMG (SDXL UNet forward, prompt-to-prompt attention
replacement, region-masked noise fusion).  See DESIGN.md."""
__version__ = "0.1.0"

_SAM = ("SamPromptEncoder", "SamMaskDecoder", "EfficientViTSam", "EfficientViTSamPredictor", "efficientvit_sam")
__all__ = list(_SAM)


def __getattr__(name):          # the segmenter's public names, imported on first use (omg_amd.sam pulls in torch and the kernels' bindings)
    if name in _SAM:
        from . import sam
        return getattr(sam, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
