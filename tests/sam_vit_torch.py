"""SAM's ViT image encoder, the whole ``Sam`` model and the predictor's flow in plain torch fp32: the oracle of omg_amd/sam_vit.py and
omg_amd/segment_anything.py.  The sibling of tests/sam_torch.py (prompt encoder, mask decoder), whose ``seed_state`` and ``checksum``
it reuses.

Written from the published architecture (Kirillov et al., "Segment Anything", 2023; the encoder is the ViTDet backbone of Li et al.,
"Exploring Plain Vision Transformer Backbones for Object Detection", 2022: non-overlapping windows with zero padding at the bottom
and right, a few global-attention blocks, decomposed relative-position terms on the unscaled query) under the parameter names of the
``segment_anything`` checkpoint layout.  ``transformers``' ``SamVisionEncoder`` is the same network under other names: ``hf_key`` maps
a key of this layout to theirs and tests/test_sam_vit.py pins the two against each other."""
import math
import re

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import sam_torch as st
from tests.sam_torch import LayerNorm2d, checksum, seed_state  # noqa: F401  (re-exported)


class PatchEmbed(nn.Module):
    def __init__(self, patch, cin, dim):
        super().__init__()
        self.proj = nn.Conv2d(cin, dim, patch, patch)

    def forward(self, x):
        return self.proj(x).permute(0, 2, 3, 1)                       # B H W C


def rel_table(q_size, k_size, rel_pos):
    """[q_size, k_size, d]: the row of ``rel_pos`` for every (query coordinate, key coordinate); the table is resampled linearly
    when its length is not 2 max(q_size, k_size) - 1."""
    n = 2 * max(q_size, k_size) - 1
    if rel_pos.shape[0] != n:
        rel_pos = F.interpolate(rel_pos.t()[None], size=n, mode="linear")[0].t()
    q = torch.arange(q_size)[:, None] * max(k_size / q_size, 1.0)
    k = torch.arange(k_size)[None, :] * max(q_size / k_size, 1.0)
    return rel_pos[(q - k + (k_size - 1) * max(q_size / k_size, 1.0)).long()]


class Attention(nn.Module):
    def __init__(self, dim, heads, size):
        super().__init__()
        self.num_heads, self.scale = heads, (dim // heads) ** -0.5
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.rel_pos_h = nn.Parameter(torch.zeros(2 * size[0] - 1, dim // heads))
        self.rel_pos_w = nn.Parameter(torch.zeros(2 * size[1] - 1, dim // heads))

    def forward(self, x):
        B, H, W, _ = x.shape
        nh = self.num_heads
        qkv = self.qkv(x).reshape(B, H * W, 3, nh, -1).permute(2, 0, 3, 1, 4)            # 3 B heads HW d
        q, k, v = qkv[0], qkv[1], qkv[2]
        s = (q * self.scale) @ k.transpose(-2, -1)                                         # B heads HW HW
        qg = q.reshape(B, nh, H, W, -1)
        bh = torch.einsum("bnhwc,hkc->bnhwk", qg, rel_table(H, H, self.rel_pos_h))     # the bias terms use the unscaled q
        bw = torch.einsum("bnhwc,wkc->bnhwk", qg, rel_table(W, W, self.rel_pos_w))
        s = (s.view(B, nh, H, W, H, W) + bh[..., :, None] + bw[..., None, :]).view(B, nh, H * W, H * W)
        o = torch.softmax(s, dim=-1) @ v
        return self.proj(o.view(B, nh, H, W, -1).permute(0, 2, 3, 1, 4).reshape(B, H, W, -1))


class MLPBlock(nn.Module):
    def __init__(self, dim, mlp_dim):
        super().__init__()
        self.lin1, self.lin2 = nn.Linear(dim, mlp_dim), nn.Linear(mlp_dim, dim)

    def forward(self, x):
        return self.lin2(F.gelu(self.lin1(x)))


class Block(nn.Module):
    def __init__(self, dim, heads, mlp_ratio, window, grid):
        super().__init__()
        self.window_size = window
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, heads, (window, window) if window else (grid, grid))
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = MLPBlock(dim, int(dim * mlp_ratio))

    def forward(self, x):
        y = self.norm1(x)
        S = self.window_size
        if S:
            B, H, W, C = y.shape
            ph, pw = (S - H % S) % S, (S - W % S) % S
            y = F.pad(y, (0, 0, 0, pw, 0, ph))                                            # zeros AFTER the norm
            Hp, Wp = H + ph, W + pw
            y = y.view(B, Hp // S, S, Wp // S, S, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, S, S, C)
            y = self.attn(y)
            y = y.view(B, Hp // S, Wp // S, S, S, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)[:, :H, :W]
        else:
            y = self.attn(y)
        x = x + y
        return x + self.mlp(self.norm2(x))


class ImageEncoderViT(nn.Module):
    def __init__(self, img_size=1024, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, out_chans=256,
                 window_size=14, global_attn_indexes=(2, 5, 8, 11)):
        super().__init__()
        self.img_size = img_size
        g = img_size // patch_size
        self.patch_embed = PatchEmbed(patch_size, in_chans, embed_dim)
        self.pos_embed = nn.Parameter(torch.zeros(1, g, g, embed_dim))
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, 0 if i in global_attn_indexes else window_size, g) for i in range(depth)])
        self.neck = nn.Sequential(nn.Conv2d(embed_dim, out_chans, 1, bias=False), LayerNorm2d(out_chans),
                                  nn.Conv2d(out_chans, out_chans, 3, padding=1, bias=False), LayerNorm2d(out_chans))
        self.trace = None                              # a dict: "patch_embed", "block{i}" (NHWC) as they are computed

    def forward(self, x):
        x = self.patch_embed(x) + self.pos_embed
        if self.trace is not None:
            self.trace["patch_embed"] = x
        for i, blk in enumerate(self.blocks):
            x = blk(x)
            if self.trace is not None:
                self.trace[f"block{i}"] = x
        return self.neck(x.permute(0, 3, 1, 2))


class Sam(nn.Module):
    mask_threshold = 0.0

    def __init__(self, image_encoder, prompt_encoder, mask_decoder, pixel_mean=(123.675, 116.28, 103.53), pixel_std=(58.395, 57.12, 57.375)):
        super().__init__()
        self.image_encoder, self.prompt_encoder, self.mask_decoder = image_encoder, prompt_encoder, mask_decoder
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std).view(-1, 1, 1), False)

    def preprocess(self, x):
        x = (x - self.pixel_mean) / self.pixel_std
        s = self.image_encoder.img_size
        return F.pad(x, (0, s - x.shape[-1], 0, s - x.shape[-2]))


def build(embed_dim, depth, num_heads, global_attn_indexes, mlp_dim=2048, img_size=1024):
    enc = ImageEncoderViT(img_size, 16, 3, embed_dim, depth, num_heads, 4.0, 256, 14, tuple(global_attn_indexes))
    g = img_size // 16
    pe, md = st.build((g, g), (img_size, img_size), mlp_dim=mlp_dim)
    return Sam(enc, pe, md).eval()


def seed_vit(module, seed):
    """``seed_state`` plus what its rules do not know of the encoder: ``pos_embed`` large enough to matter (1 / sqrt(fan_in) of a
    [1, 64, 64, D] tensor is nothing), LayerNorm2d weights of the neck near 1, relative-position tables at 1 / sqrt(d).  fp16 grid."""
    seed_state(module, seed)
    rs = np.random.RandomState(seed + 7919)
    with torch.no_grad():
        for key, t in module.state_dict().items():
            if re.search(r"(^|\.)pos_embed$", key):
                t.copy_(torch.from_numpy(0.5 * rs.standard_normal(tuple(t.shape)).astype(np.float32)).half().float())
            elif re.search(r"(^|\.)neck\.[13]\.weight$", key):
                t.copy_(torch.from_numpy(1.0 + 0.2 * rs.standard_normal(tuple(t.shape)).astype(np.float32)).half().float())
    return module


def hf_key(key):
    """``image_encoder.*`` key of the segment_anything layout (without the prefix) -> key of transformers' ``SamVisionEncoder``."""
    k = key.replace("patch_embed.proj.", "patch_embed.projection.")
    k = re.sub(r"^blocks\.(\d+)\.norm([12])\.", r"layers.\1.layer_norm\2.", k)
    k = re.sub(r"^blocks\.", "layers.", k)
    k = re.sub(r"^neck\.0\.", "neck.conv1.", k)
    k = re.sub(r"^neck\.1\.", "neck.layer_norm1.", k)
    k = re.sub(r"^neck\.2\.", "neck.conv2.", k)
    k = re.sub(r"^neck\.3\.", "neck.layer_norm2.", k)
    return k


# ------------------------------------------------------------------------------------------------ the predictor's flow
def resize_longest(image, side=1024):
    """HWC uint8 -> HWC uint8 with the long side at ``side``, bilinear through PIL."""
    from PIL import Image
    th, tw = st.get_preprocess_shape(image.shape[0], image.shape[1], side)
    return np.array(Image.fromarray(np.ascontiguousarray(image)).resize((tw, th), Image.BILINEAR))


def apply_coords(coords, original_size, side=1024):
    oh, ow = original_size
    nh, nw = st.get_preprocess_shape(oh, ow, side)
    c = np.array(coords, dtype=float, copy=True)
    c[..., 0] = c[..., 0] * (nw / ow)
    c[..., 1] = c[..., 1] * (nh / oh)
    return c


@torch.no_grad()
def embed(sam, image):
    """HWC uint8 RGB -> (embedding [1, 256, 64, 64], input_size)."""
    r = resize_longest(image, sam.image_encoder.img_size)
    x = torch.from_numpy(np.ascontiguousarray(r)).permute(2, 0, 1)[None].float()
    return sam.image_encoder(sam.preprocess(x)), tuple(r.shape[:2])


@torch.no_grad()
def predict(sam, feat, input_size, original_size, points=None, boxes=None, multimask=False):
    """Prompts in the input frame -> (final logits at original_size, iou, low-resolution logits)."""
    sparse, dense = sam.prompt_encoder(points=points, boxes=boxes, masks=None)
    low, iou = sam.mask_decoder(feat, sam.prompt_encoder.get_dense_pe(), sparse, dense, multimask)
    return st.postprocess_masks(low, sam.image_encoder.img_size, input_size, original_size), iou, low


# ------------------------------------------------------------------------------------------------ the fixture's models (tests/golden/sam_vit_golden.npz)
def seeded_oracle(gold, name):
    """The fp32 ``Sam`` of the fixture's model ``name`` ("d64" | "d80") with the weights the fixture was made with."""
    c = {k: gold[f"{name}.cfg_{k}"] for k in ("embed_dim", "depth", "heads", "mlp_dim", "seed_enc", "seed_pe", "seed_md")}
    sam = build(int(c["embed_dim"]), int(c["depth"]), int(c["heads"]), [int(v) for v in gold[f"{name}.cfg_global"]], mlp_dim=int(c["mlp_dim"]))
    seed_vit(sam.image_encoder, int(c["seed_enc"]))
    seed_state(sam.prompt_encoder, int(c["seed_pe"]))
    seed_state(sam.mask_decoder, int(c["seed_md"]))
    return sam


def narrow_model(gold, name, dtype=torch.float16, device=None):
    """omg_amd.segment_anything.Sam of the fixture's model ``name``, loaded from the oracle's state dict."""
    from omg_amd import sam as osam
    from omg_amd import segment_anything as sa
    from omg_amd.sam_vit import SamImageEncoderViT
    ref = seeded_oracle(gold, name)
    enc = SamImageEncoderViT(embed_dim=int(gold[f"{name}.cfg_embed_dim"]), depth=int(gold[f"{name}.cfg_depth"]), num_heads=int(gold[f"{name}.cfg_heads"]),
                             global_attn_indexes=tuple(int(v) for v in gold[f"{name}.cfg_global"]), dtype=dtype, device=device)
    m = sa.Sam(enc, osam.SamPromptEncoder(256, (64, 64), (1024, 1024), 16, dtype=dtype, device=device),
               osam.SamMaskDecoder(256, 3, 2, 8, int(gold[f"{name}.cfg_mlp_dim"]), 3, 256, dtype=dtype, device=device))
    m.load_state_dict(ref.state_dict(), strict=True)
    return m
