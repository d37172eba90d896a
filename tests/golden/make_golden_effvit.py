"""Golden vectors of the EfficientViT-SAM image encoder, produced by the REFERENCE's own classes on the CPU in fp32.

    python tests/golden/make_golden_effvit.py        (needs /root/reference; writes effvit_golden.npz next to itself)

``src/efficientvit/models/efficientvit/sam.py`` imports ``segment_anything`` and ``torchvision`` at module top (neither is installed;
``SamNeck`` and ``EfficientViTSamImageEncoder`` need neither): empty stand-ins are registered first.  The package ``__init__`` files
of ``src/efficientvit`` import torchvision too, so bare package objects take their place (as make_golden.py does for LiteMLA) and
only models/utils/*, models/nn/{act,norm,ops}.py, models/efficientvit/{backbone,sam}.py are executed.

What is written:
  cfg_*            the narrow config (this project's EfficientViTSamConfig fields) the fixture was made with
  sd.<key>         the state dict of the reference's EfficientViTSamImageEncoder (its own key layout), seeded, BatchNorm running
                   statistics away from the identity; values rounded to the fp16 grid so that an fp16 model loads them exactly
  x                the input [1, 3, 128, 128] (fp16-representable values)
  stage0 .. stage4 the backbone's stage outputs
  neck_mid         the neck after its fusion (conv + bicubic upsample of three stages, summed) and middle blocks: every pixel of the 64 x 64 grid
  neck, out        the neck's 256-channel output and the embedding after LayerNorm2d, at the pixels [::8, ::8] (the full maps are 4 MiB each)
  params_l0/l1/l2  parameter counts of the image encoders that the reference's efficientvit_sam_l0 / l1 / l2 construct
"""
import importlib
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

# the narrow model: every block type of the l-series (ResBlock; FusedMBConv stride 2 and 1; MBConv stride 2 and 1; EfficientViTBlock),
# three neck inputs at 16 x 16, 8 x 8 and 4 x 4 for a 128 x 128 image
NARROW = dict(width_list=[8, 8, 16, 24, 32], depth_list=[1, 1, 1, 1, 1], qkv_dim=16,
              neck_fids=["stage4", "stage3", "stage2"], head_width=8, head_depth=1, neck_expand=1, neck_middle="fmb")
SUB = 8


def install_stand_ins():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)
        sys.modules[name] = m
        parent, _, leaf = name.rpartition(".")
        if parent:
            setattr(sys.modules[parent], leaf, m)
        return m

    class _Module(nn.Module):              # a constructor that takes anything and holds nothing
        def __init__(self, *a, **k):
            super().__init__()

    class _Any:
        def __init__(self, *a, **k):
            pass

    mod("torchvision")
    mod("torchvision.transforms", Compose=_Any, ToTensor=_Any, Normalize=_Any)
    mod("torchvision.transforms.functional", resize=None, to_pil_image=None)
    mod("segment_anything", SamAutomaticMaskGenerator=_Any)
    mod("segment_anything.modeling", MaskDecoder=_Module, PromptEncoder=_Module, TwoWayTransformer=_Module)
    mod("segment_anything.modeling.mask_decoder", MaskDecoder=_Module)
    mod("segment_anything.modeling.prompt_encoder", PromptEncoder=_Module)
    mod("segment_anything.utils")
    mod("segment_anything.utils.amg", build_all_layer_point_grids=None)
    mod("segment_anything.utils.transforms", ResizeLongestSide=_Any)


def import_reference():
    for name, sub in [("src.efficientvit", "src/efficientvit"), ("src.efficientvit.models", "src/efficientvit/models"),
                      ("src.efficientvit.models.nn", "src/efficientvit/models/nn"),
                      ("src.efficientvit.models.efficientvit", "src/efficientvit/models/efficientvit")]:
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [os.path.join(REF, sub)]
            sys.modules[name] = m
    nn_pkg = sys.modules["src.efficientvit.models.nn"]
    for leaf in ("act", "norm", "ops"):     # what the nn package's __init__ would have re-exported
        m = importlib.import_module(f"src.efficientvit.models.nn.{leaf}")
        for n in m.__all__:
            setattr(nn_pkg, n, getattr(m, n))
    backbone = importlib.import_module("src.efficientvit.models.efficientvit.backbone")
    sam = importlib.import_module("src.efficientvit.models.efficientvit.sam")
    # efficientvit_sam_l* import their backbone recipe under the package's installed name
    for name in ("efficientvit", "efficientvit.models", "efficientvit.models.efficientvit"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["efficientvit.models.efficientvit.backbone"] = backbone
    return backbone, sam


def seed_model(m, seed):
    """Kaiming-scaled convolutions (activations stay O(1) through the depth), BatchNorm affine and running statistics away from the
    identity, everything on the fp16 grid."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, mod in m.named_modules():
            if isinstance(mod, nn.Conv2d):
                fan_in = mod.weight[0].numel()
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (1.5 / fan_in) ** 0.5)
                if mod.bias is not None:
                    mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
            elif isinstance(mod, nn.BatchNorm2d):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
                mod.running_mean.copy_(0.2 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
            elif isinstance(mod, nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
        for t in list(m.parameters()) + [b for b in m.buffers() if b.dtype.is_floating_point]:
            t.copy_(t.half().float())


def main():
    install_stand_ins()
    backbone, sam = import_reference()
    out = {}
    for v in ("l0", "l1", "l2"):
        enc = getattr(sam, f"efficientvit_sam_{v}")().image_encoder
        out[f"params_{v}"] = np.array(sum(p.numel() for p in enc.parameters()), dtype=np.int64)
        print(v, int(out[f"params_{v}"]), "parameters")

    c = NARROW
    bb = backbone.EfficientViTLargeBackbone(width_list=c["width_list"], depth_list=c["depth_list"], qkv_dim=c["qkv_dim"])
    neck = sam.SamNeck(fid_list=c["neck_fids"], in_channel_list=[c["width_list"][int(f[-1])] for f in c["neck_fids"]],
                       head_width=c["head_width"], head_depth=c["head_depth"], expand_ratio=c["neck_expand"], middle_op=c["neck_middle"])
    enc = sam.EfficientViTSamImageEncoder(bb, neck).eval()
    seed_model(enc, 20)
    kinds = {type(m).__name__ for m in enc.modules()}
    assert {"ResBlock", "FusedMBConv", "MBConv", "EfficientViTBlock", "LiteMLA", "UpSampleLayer", "LayerNorm2d"} <= kinds, kinds
    x = torch.randn(1, 3, 128, 128, generator=torch.Generator().manual_seed(21)).half().float()
    mid = {}
    h = enc.neck.middle.register_forward_hook(lambda m_, i_, o_: mid.__setitem__("y", o_))
    with torch.no_grad():
        feats = enc.backbone(x)
        stages = {k: v.clone() for k, v in feats.items() if k.startswith("stage") and k != "stage_final"}
        neck_out = enc.neck(feats)["sam_encoder"]
        y = enc.norm(neck_out)
        assert torch.equal(y, enc(x))
    h.remove()
    for k, v in c.items():                 # lists of integers, integers and strings; neck_fids as stage numbers
        out["cfg_" + k] = np.array([int(f[-1]) for f in v] if k == "neck_fids" else v)
    out["cfg_sub"] = np.array(SUB)
    out["x"] = x.numpy()
    for k, v in stages.items():
        out[k] = v.numpy()
    out["neck_mid"] = mid["y"].numpy()
    out["neck"] = neck_out[:, :, ::SUB, ::SUB].contiguous().numpy()
    out["out"] = y[:, :, ::SUB, ::SUB].contiguous().numpy()
    for k, v in enc.state_dict().items():
        out["sd." + k] = v.numpy()
    for k, v in out.items():
        assert v.dtype in (np.float32, np.int64) or v.dtype.kind == "U", (k, v.dtype)
    path = os.path.join(HERE, "effvit_golden.npz")
    np.savez_compressed(path, **out)
    print("effvit_golden.npz:", len(out), "arrays,", os.path.getsize(path), "bytes;",
          {k: (tuple(v.shape), float(np.abs(v).max())) for k, v in out.items() if k.startswith(("stage", "neck", "out"))})


if __name__ == "__main__":
    main()
