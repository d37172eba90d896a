"""Golden vectors of the six-stage (xl) EfficientViT-SAM image encoder, produced by the REFERENCE's own classes on the CPU in fp32, with
the norm eps that the reference's ``create_sam_model`` sets (``set_norm_eps(model, 1e-6)``, sam_model_zoo.py:44).

    python tests/golden/make_golden_effvit_xl.py        (needs the reference checkout make_golden_effvit.py points to; writes effvit_xl_golden.npz next to itself)

The stand-ins and the import of the reference are those of make_golden_effvit.py.  The model is narrow but has the xl topology: six
stages, ``depth_list[0] == 0`` (the stem alone, as xl0), FusedMBConv in stages 1-3, ``att@3`` blocks (LiteMLA with scales (3,)) behind
an MBConv downsample at ``expand x 4`` in stages 4 and 5, a neck over stages 5, 4, 3 with ``expand_ratio`` 4.  A 128 x 128 input puts the
neck's inputs at 8 x 8, 4 x 4 and 2 x 2.

Seeding is ``seed_model`` of the sibling with one change: in every BatchNorm a tenth of the channels (at least one) gets a running
variance of about 1e-4, and those channels' ``weight`` is scaled by sqrt(var), so that activations stay O(1) while eps = 1e-6 and
eps = 1e-5 give results 4 % apart in those channels.

What is written:
  cfg_*              the narrow config (EfficientViTSamConfig fields of this project, block / expand / fewer_norm lists included), cfg_eps
  sd.<key>           the state dict of the reference's EfficientViTSamImageEncoder, values on the fp16 grid
  x                  the input [1, 3, 128, 128]
  stage0 .. stage5   the backbone's stage outputs
  neck_mid           the neck after its fusion and middle blocks, every pixel of the 64 x 64 grid
  neck, out          the neck's 256-channel output and the embedding after LayerNorm2d at the pixels [::8, ::8]
  params_xl0 / xl1   parameter counts of the image encoders that the reference's efficientvit_sam_xl0 / _xl1 construct
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_effvit as ge          # noqa: E402

NARROW_XL = dict(width_list=[8, 8, 8, 16, 16, 32], depth_list=[0, 1, 1, 1, 1, 1], block_list=["res", "fmb", "fmb", "fmb", "att@3", "att@3"],
                 expand_list=[1, 4, 4, 4, 4, 6], fewer_norm_list=[False, False, False, False, True, True], qkv_dim=16,
                 neck_fids=["stage5", "stage4", "stage3"], head_width=8, head_depth=2, neck_expand=4, neck_middle="fmb")
SUB = 8
EPS = 1e-6
SEED_MODEL, SEED_VAR, SEED_X = 40, 41, 42


def seed_model_xl(m, seed, seed_var):
    """seed_model, then small running variances in a tenth of every BatchNorm's channels (weight scaled to keep the output O(1))."""
    ge.seed_model(m, seed)
    g = torch.Generator().manual_seed(seed_var)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                c = mod.running_var.numel()
                idx = torch.randperm(c, generator=g)[:max(1, c // 10)]
                var = 1e-4 * (1.0 + 0.5 * torch.rand(idx.numel(), generator=g))
                mod.running_var[idx] = var.half().float()
                mod.weight[idx] = (mod.weight[idx] * mod.running_var[idx].sqrt()).half().float()


def build_encoder(backbone, sam):
    c = NARROW_XL
    bb = backbone.EfficientViTLargeBackbone(width_list=c["width_list"], depth_list=c["depth_list"], block_list=c["block_list"],
                                            expand_list=c["expand_list"], fewer_norm_list=c["fewer_norm_list"], qkv_dim=c["qkv_dim"])
    neck = sam.SamNeck(fid_list=c["neck_fids"], in_channel_list=[c["width_list"][int(f[-1])] for f in c["neck_fids"]],
                       head_width=c["head_width"], head_depth=c["head_depth"], expand_ratio=c["neck_expand"], middle_op=c["neck_middle"])
    enc = sam.EfficientViTSamImageEncoder(bb, neck).eval()
    seed_model_xl(enc, SEED_MODEL, SEED_VAR)
    return enc


def main():
    ge.install_stand_ins()
    backbone, sam = ge.import_reference()
    set_norm_eps = sys.modules["src.efficientvit.models.nn.norm"].set_norm_eps
    out = {}
    for v in ("xl0", "xl1"):
        enc = getattr(sam, f"efficientvit_sam_{v}")().image_encoder
        out[f"params_{v}"] = np.array(sum(p.numel() for p in enc.parameters()), dtype=np.int64)
        print(v, int(out[f"params_{v}"]), "parameters")
        del enc

    c = NARROW_XL
    enc = build_encoder(backbone, sam)
    set_norm_eps(enc, EPS)
    assert all(m.eps == EPS for m in enc.modules() if isinstance(m, (nn.BatchNorm2d, nn.LayerNorm)))
    assert isinstance(enc.norm, nn.LayerNorm) and enc.norm.eps == EPS
    kinds = {type(m).__name__ for m in enc.modules()}
    assert {"FusedMBConv", "MBConv", "EfficientViTBlock", "LiteMLA", "UpSampleLayer", "LayerNorm2d"} <= kinds and "ResBlock" not in kinds, kinds
    assert all(m.aggreg[0][0].kernel_size == (3, 3) for m in enc.modules() if type(m).__name__ == "LiteMLA")
    x = torch.randn(1, 3, 128, 128, generator=torch.Generator().manual_seed(SEED_X)).half().float()
    mid = {}
    h = enc.neck.middle.register_forward_hook(lambda m_, i_, o_: mid.__setitem__("y", o_))
    with torch.no_grad():
        feats = enc.backbone(x)
        stages = {k: v.clone() for k, v in feats.items() if k.startswith("stage") and k != "stage_final"}
        neck_out = enc.neck(feats)["sam_encoder"]
        y = enc.norm(neck_out)
        assert torch.equal(y, enc(x))
    h.remove()
    assert [tuple(stages[f].shape[-2:]) for f in c["neck_fids"]] == [(2, 2), (4, 4), (8, 8)]
    for k, v in c.items():
        out["cfg_" + k] = np.array([int(f[-1]) for f in v] if k == "neck_fids" else v)
    out["cfg_sub"], out["cfg_eps"] = np.array(SUB), np.array(EPS)
    out["x"] = x.numpy()
    for k, v in stages.items():
        out[k] = v.numpy()
    out["neck_mid"] = mid["y"].numpy()
    out["neck"] = neck_out[:, :, ::SUB, ::SUB].contiguous().numpy()
    out["out"] = y[:, :, ::SUB, ::SUB].contiguous().numpy()
    for k, v in enc.state_dict().items():
        out["sd." + k] = v.numpy()
    for k, v in out.items():
        assert v.dtype in (np.float32, np.float64, np.int64, np.bool_) or v.dtype.kind == "U", (k, v.dtype)
    path = os.path.join(HERE, "effvit_xl_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("effvit_xl_golden.npz:", len(out), "arrays,", size, "bytes;",
          {k: (tuple(v.shape), float(np.abs(v).max())) for k, v in out.items() if k.startswith(("stage", "neck", "out"))})
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
