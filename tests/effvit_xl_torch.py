"""Helpers of the xl (six-stage) EfficientViT-SAM tests: the fixture loaders of tests/golden/effvit_xl_golden.npz and sam_xl_golden.npz,
and tests/effvit_torch.TorchEncoder with LiteMLA's ``proj.norm`` evaluated at the module's own eps (the sibling's oracle call leaves
the BatchNorm eps at its default of 1e-5, which the l-series fixture was made with; everything else of the class is used as it is)."""
import os

import numpy as np
import torch

from omg_amd import efficientvit as ev
from tests.effvit_torch import TorchEncoder, build_from_fixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD_ENC = os.path.join(GOLDEN, "effvit_xl_golden.npz")
GOLD_SAM = os.path.join(GOLDEN, "sam_xl_golden.npz")


class XlTorchEncoder(TorchEncoder):
    def litemla(self, blk, x):
        if self.rounded:
            return blk(x, residual=True)
        from oracle import litemla as ol
        sd = {k: v.float() for k, v in blk.state_dict().items()}
        return x + ol.litemla_forward(sd, x, dim=blk.dim, scales=blk.scales, bn_eps=blk.proj.norm.eps)


def load_fixture_xl(path=GOLD_ENC):
    """-> (npz, config with the recorded block / expand / fewer_norm lists, state dict, vectors, subsampling stride)."""
    g = np.load(path)
    cfg = ev.EfficientViTSamConfig(width_list=tuple(g["cfg_width_list"].tolist()), depth_list=tuple(g["cfg_depth_list"].tolist()),
                                   block_list=tuple(str(b) for b in g["cfg_block_list"]), expand_list=tuple(g["cfg_expand_list"].tolist()),
                                   fewer_norm_list=tuple(bool(b) for b in g["cfg_fewer_norm_list"]), qkv_dim=int(g["cfg_qkv_dim"]),
                                   neck_fids=tuple(g["cfg_neck_fids"].tolist()), head_width=int(g["cfg_head_width"]),
                                   head_depth=int(g["cfg_head_depth"]), neck_expand=int(g["cfg_neck_expand"]),
                                   neck_middle=str(g["cfg_neck_middle"]), fused_aggreg=True)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    vec = {k: torch.from_numpy(g[k]) for k in g.files if k == "x" or k.startswith(("stage", "neck", "out"))}
    return g, cfg, sd, vec, int(g["cfg_sub"])


def build_xl(cfg, sd, dtype, device, eps=1e-6):
    """The narrow xl encoder with the fixture's weights and, unless ``eps`` is None, set_norm_eps(model, eps)."""
    from omg_amd.sam import set_norm_eps
    m = build_from_fixture(cfg, sd, dtype, device)
    if eps is not None:
        set_norm_eps(m, eps)
    return m


def narrow_sam_xl(gold, dtype=torch.float16, device=None):
    """omg_amd.sam.EfficientViTSam of sam_xl_golden.npz: the narrow xl encoder, the seeded prompt encoder and decoder, loaded as one
    checkpoint-shaped state dict; set_norm_eps(model, 1e-6) on the whole model, as create_sam_model does."""
    from omg_amd import sam
    from tests import sam_torch as st
    _, cfg, enc_sd, _, _ = load_fixture_xl()
    size = tuple(int(v) for v in gold["cfg_image_size"])
    m = sam.EfficientViTSam(ev.EfficientViTSamImageEncoder(cfg, dtype=dtype, device=device),
                            sam.SamPromptEncoder(256, (64, 64), (size[0], size[0]), 16, dtype=dtype, device=device),
                            sam.SamMaskDecoder(256, 3, 2, 8, int(gold["cfg_mlp_dim"]), 3, 256, dtype=dtype, device=device), image_size=size)
    sam.set_norm_eps(m, float(gold["cfg_eps"]))
    pe, md = st.seeded_oracle(gold)
    sd = {"image_encoder." + k: v for k, v in enc_sd.items()}
    sd.update({"prompt_encoder." + k: v for k, v in pe.state_dict().items()})
    sd.update({"mask_decoder." + k: v for k, v in md.state_dict().items()})
    m.load_state_dict(sd, strict=True)
    return m
