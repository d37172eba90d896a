"""SAM's prompt encoder, mask decoder and predictor maths in plain torch fp32: the oracle of omg_amd/sam.py.

Written from the published architecture (Kirillov et al., "Segment Anything", 2023) under the parameter names of the
``segment_anything`` checkpoint layout (``prompt_encoder.*`` / ``mask_decoder.*`` of an ``efficientvit_sam_*.pt`` file); the
constructors take the arguments ``segment_anything.modeling`` takes, so the reference's ``EfficientViTSam`` accepts these classes.
``transformers``' ``SamPromptEncoder`` / ``SamMaskDecoder`` are the same networks under other names: ``hf_key`` maps a key of this
layout to theirs and tests/test_sam.py pins the two against each other.

``seed_state`` fills a module from numpy's legacy MT19937 stream (stable across numpy versions), on the fp16 grid: a decoder at SAM's
fixed width of 256 has 2 M parameters, more than a committed fixture may hold, so fixtures keep the seed and per-key checksums."""
import math
import re

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class LayerNorm2d(nn.Module):
    def __init__(self, c, eps=1e-6):
        super().__init__()
        self.weight, self.bias, self.eps = nn.Parameter(torch.ones(c)), nn.Parameter(torch.zeros(c)), eps

    def forward(self, x):
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        return self.weight[:, None, None] * ((x - u) / torch.sqrt(s + self.eps)) + self.bias[:, None, None]


class PositionEmbeddingRandom(nn.Module):
    def __init__(self, num_pos_feats=64, scale=None):
        super().__init__()
        self.register_buffer("positional_encoding_gaussian_matrix", (scale or 1.0) * torch.randn(2, num_pos_feats))

    def _pe(self, coords):                              # coords in [0, 1]^2, (x, y) last
        c = (2 * coords - 1) @ self.positional_encoding_gaussian_matrix
        c = 2 * math.pi * c
        return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)

    def forward(self, size):
        h, w = size
        g = torch.ones(h, w, dtype=torch.float32)
        y = (g.cumsum(0) - 0.5) / h
        x = (g.cumsum(1) - 0.5) / w
        return self._pe(torch.stack([x, y], dim=-1)).permute(2, 0, 1)          # C x H x W

    def forward_with_coords(self, coords, image_size):
        c = coords.clone()
        c[..., 0] = c[..., 0] / image_size[1]
        c[..., 1] = c[..., 1] / image_size[0]
        return self._pe(c.float())


class PromptEncoder(nn.Module):
    def __init__(self, embed_dim, image_embedding_size, input_image_size, mask_in_chans, activation=nn.GELU):
        super().__init__()
        self.embed_dim, self.image_embedding_size, self.input_image_size = embed_dim, image_embedding_size, input_image_size
        self.pe_layer = PositionEmbeddingRandom(embed_dim // 2)
        self.point_embeddings = nn.ModuleList([nn.Embedding(1, embed_dim) for _ in range(4)])
        self.not_a_point_embed = nn.Embedding(1, embed_dim)
        self.mask_downscaling = nn.Sequential(
            nn.Conv2d(1, mask_in_chans // 4, 2, 2), LayerNorm2d(mask_in_chans // 4), activation(),
            nn.Conv2d(mask_in_chans // 4, mask_in_chans, 2, 2), LayerNorm2d(mask_in_chans), activation(),
            nn.Conv2d(mask_in_chans, embed_dim, 1))
        self.no_mask_embed = nn.Embedding(1, embed_dim)

    def get_dense_pe(self):
        return self.pe_layer(self.image_embedding_size).unsqueeze(0)

    def _embed_points(self, points, labels, pad):
        points = points + 0.5
        if pad:
            points = torch.cat([points, torch.zeros(points.shape[0], 1, 2)], dim=1)
            labels = torch.cat([labels, -torch.ones(labels.shape[0], 1, dtype=labels.dtype)], dim=1)
        e = self.pe_layer.forward_with_coords(points, self.input_image_size)
        e = torch.where((labels == -1)[..., None], torch.zeros_like(e), e)
        e = e + (labels == -1)[..., None] * self.not_a_point_embed.weight
        e = e + (labels == 0)[..., None] * self.point_embeddings[0].weight
        e = e + (labels == 1)[..., None] * self.point_embeddings[1].weight
        return e

    def _embed_boxes(self, boxes):
        c = (boxes + 0.5).reshape(-1, 2, 2)
        e = self.pe_layer.forward_with_coords(c, self.input_image_size)
        e[:, 0, :] += self.point_embeddings[2].weight[0]
        e[:, 1, :] += self.point_embeddings[3].weight[0]
        return e

    def forward(self, points, boxes, masks):
        bs = points[0].shape[0] if points is not None else boxes.shape[0] if boxes is not None else masks.shape[0] if masks is not None else 1
        sparse = torch.empty(bs, 0, self.embed_dim)
        if points is not None:
            sparse = torch.cat([sparse, self._embed_points(points[0].float(), points[1], pad=boxes is None)], dim=1)
        if boxes is not None:
            sparse = torch.cat([sparse, self._embed_boxes(boxes.float())], dim=1)
        if masks is not None:
            dense = self.mask_downscaling(masks)
        else:
            dense = self.no_mask_embed.weight.reshape(1, -1, 1, 1).expand(bs, -1, *self.image_embedding_size)
        return sparse, dense


class Attention(nn.Module):
    def __init__(self, embedding_dim, num_heads, downsample_rate=1):
        super().__init__()
        self.internal_dim, self.num_heads = embedding_dim // downsample_rate, num_heads
        self.q_proj = nn.Linear(embedding_dim, self.internal_dim)
        self.k_proj = nn.Linear(embedding_dim, self.internal_dim)
        self.v_proj = nn.Linear(embedding_dim, self.internal_dim)
        self.out_proj = nn.Linear(self.internal_dim, embedding_dim)

    def forward(self, q, k, v):
        def split(x):
            b, n, c = x.shape
            return x.reshape(b, n, self.num_heads, c // self.num_heads).transpose(1, 2)
        q, k, v = split(self.q_proj(q)), split(self.k_proj(k)), split(self.v_proj(v))
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1]), dim=-1)
        o = (a @ v).transpose(1, 2)
        return self.out_proj(o.reshape(o.shape[0], o.shape[1], -1))


class MLPBlock(nn.Module):
    def __init__(self, embedding_dim, mlp_dim):
        super().__init__()
        self.lin1, self.lin2 = nn.Linear(embedding_dim, mlp_dim), nn.Linear(mlp_dim, embedding_dim)

    def forward(self, x):
        return self.lin2(F.relu(self.lin1(x)))


class TwoWayAttentionBlock(nn.Module):
    def __init__(self, embedding_dim, num_heads, mlp_dim, attention_downsample_rate, skip_first_layer_pe):
        super().__init__()
        self.self_attn = Attention(embedding_dim, num_heads)
        self.norm1 = nn.LayerNorm(embedding_dim)
        self.cross_attn_token_to_image = Attention(embedding_dim, num_heads, attention_downsample_rate)
        self.norm2 = nn.LayerNorm(embedding_dim)
        self.mlp = MLPBlock(embedding_dim, mlp_dim)
        self.norm3 = nn.LayerNorm(embedding_dim)
        self.norm4 = nn.LayerNorm(embedding_dim)
        self.cross_attn_image_to_token = Attention(embedding_dim, num_heads, attention_downsample_rate)
        self.skip_first_layer_pe = skip_first_layer_pe

    def forward(self, queries, keys, query_pe, key_pe):
        if self.skip_first_layer_pe:
            queries = self.self_attn(queries, queries, queries)
        else:
            q = queries + query_pe
            queries = queries + self.self_attn(q, q, queries)
        queries = self.norm1(queries)
        queries = self.norm2(queries + self.cross_attn_token_to_image(queries + query_pe, keys + key_pe, keys))
        queries = self.norm3(queries + self.mlp(queries))
        keys = self.norm4(keys + self.cross_attn_image_to_token(keys + key_pe, queries + query_pe, queries))
        return queries, keys


class TwoWayTransformer(nn.Module):
    def __init__(self, depth, embedding_dim, num_heads, mlp_dim, activation=nn.ReLU, attention_downsample_rate=2):
        super().__init__()
        self.layers = nn.ModuleList([TwoWayAttentionBlock(embedding_dim, num_heads, mlp_dim, attention_downsample_rate, i == 0)
                                     for i in range(depth)])
        self.final_attn_token_to_image = Attention(embedding_dim, num_heads, attention_downsample_rate)
        self.norm_final_attn = nn.LayerNorm(embedding_dim)
        self.trace = None                              # a list: (queries, keys) after every layer and after the final attention

    def forward(self, image_embedding, image_pe, point_embedding):
        keys = image_embedding.flatten(2).permute(0, 2, 1)
        key_pe = image_pe.flatten(2).permute(0, 2, 1)
        queries = point_embedding
        for layer in self.layers:
            queries, keys = layer(queries, keys, point_embedding, key_pe)
            if self.trace is not None:
                self.trace.append((queries, keys))
        queries = self.norm_final_attn(queries + self.final_attn_token_to_image(queries + point_embedding, keys + key_pe, keys))
        if self.trace is not None:
            self.trace.append((queries, keys))
        return queries, keys


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        dims = [input_dim] + [hidden_dim] * (num_layers - 1) + [output_dim]
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x):
        for i, l in enumerate(self.layers):
            x = F.relu(l(x)) if i < len(self.layers) - 1 else l(x)
        return x


class MaskDecoder(nn.Module):
    def __init__(self, *, transformer_dim, transformer, num_multimask_outputs=3, activation=nn.GELU, iou_head_depth=3, iou_head_hidden_dim=256):
        super().__init__()
        self.transformer = transformer
        self.num_mask_tokens = num_multimask_outputs + 1
        self.iou_token = nn.Embedding(1, transformer_dim)
        self.mask_tokens = nn.Embedding(self.num_mask_tokens, transformer_dim)
        self.output_upscaling = nn.Sequential(
            nn.ConvTranspose2d(transformer_dim, transformer_dim // 4, 2, 2), LayerNorm2d(transformer_dim // 4), activation(),
            nn.ConvTranspose2d(transformer_dim // 4, transformer_dim // 8, 2, 2), activation())
        self.output_hypernetworks_mlps = nn.ModuleList(MLP(transformer_dim, transformer_dim, transformer_dim // 8, 3)
                                                       for _ in range(self.num_mask_tokens))
        self.iou_prediction_head = MLP(transformer_dim, iou_head_hidden_dim, self.num_mask_tokens, iou_head_depth)

    def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output):
        n = sparse_prompt_embeddings.shape[0]
        tokens = torch.cat([self.iou_token.weight, self.mask_tokens.weight], dim=0)
        tokens = torch.cat([tokens.unsqueeze(0).expand(n, -1, -1), sparse_prompt_embeddings], dim=1)
        src = torch.repeat_interleave(image_embeddings, n, dim=0) + dense_prompt_embeddings
        pos = torch.repeat_interleave(image_pe, n, dim=0)
        b, c, h, w = src.shape
        hs, src = self.transformer(src, pos, tokens)
        up = self.output_upscaling(src.transpose(1, 2).reshape(b, c, h, w))
        hyper = torch.stack([m(hs[:, 1 + i, :]) for i, m in enumerate(self.output_hypernetworks_mlps)], dim=1)
        b, c, h, w = up.shape
        masks = (hyper @ up.reshape(b, c, h * w)).reshape(b, -1, h, w)
        iou = self.iou_prediction_head(hs[:, 0, :])
        s = slice(1, None) if multimask_output else slice(0, 1)
        return masks[:, s], iou[:, s]


def build(image_embedding_size=(64, 64), input_image_size=(1024, 1024), mlp_dim=2048, iou_head_hidden_dim=256, dim=256):
    """(PromptEncoder, MaskDecoder) with the arguments the reference's efficientvit_sam_l* pass."""
    pe = PromptEncoder(embed_dim=dim, image_embedding_size=image_embedding_size, input_image_size=input_image_size, mask_in_chans=16)
    md = MaskDecoder(num_multimask_outputs=3, transformer=TwoWayTransformer(depth=2, embedding_dim=dim, mlp_dim=mlp_dim, num_heads=8),
                     transformer_dim=dim, iou_head_depth=3, iou_head_hidden_dim=iou_head_hidden_dim)
    return pe.eval(), md.eval()


def seed_state(module, seed):
    """Fill every parameter and floating buffer, in state-dict order, from ``np.random.RandomState(seed)``: matrices and convolutions
    at 1 / sqrt(fan_in), norm weights near 1, biases and embeddings small enough / large enough to matter; all on the fp16 grid."""
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for key, t in module.state_dict().items():
            if not t.dtype.is_floating_point:
                continue
            z = torch.from_numpy(rs.standard_normal(tuple(t.shape)).astype(np.float32))
            if re.search(r"gaussian_matrix$|(^|\.)(point_embeddings\.\d|not_a_point_embed|no_mask_embed|iou_token|mask_tokens)\.weight$", key):
                v = z
            elif "norm" in key or re.search(r"(output_upscaling\.1|mask_downscaling\.[14])\.", key):
                v = 1.0 + 0.2 * z if key.endswith("weight") else 0.1 * z
            elif key.endswith("bias"):
                v = 0.1 * z
            elif "output_upscaling" in key:
                v = z / math.sqrt(t.shape[0])                # ConvTranspose2d [Cin, Cout, 2, 2]: one tap per output pixel
            else:
                v = z / math.sqrt(t[0].numel())
            t.copy_(v.half().float())
    return module


def checksum(t):
    """A float64 fingerprint of a tensor: (sum, sum of |x| weighted by position)."""
    a = t.detach().double().flatten()
    return np.array([a.sum().item(), (a.abs() * torch.linspace(1.0, 2.0, a.numel(), dtype=torch.float64)).sum().item()])


# ------------------------------------------------------------------------------------------------ the transformers names
def hf_key(key):
    """``prompt_encoder.*`` / ``mask_decoder.*`` key of the segment_anything layout -> (which, key) of transformers' ``SamPromptEncoder``
    / ``SamMaskDecoder`` (which = "prompt_encoder" | "mask_decoder")."""
    which, _, k = key.partition(".")
    if which == "prompt_encoder":
        k = k.replace("pe_layer.positional_encoding_gaussian_matrix", "shared_embedding.positional_embedding")
        k = re.sub(r"^point_embeddings\.", "point_embed.", k)
        for a, b in (("0", "conv1"), ("1", "layer_norm1"), ("3", "conv2"), ("4", "layer_norm2"), ("6", "conv3")):
            k = re.sub(rf"^mask_downscaling\.{a}\.", f"mask_embed.{b}.", k)
        return which, k
    k = re.sub(r"\.norm([1-4])\.", r".layer_norm\1.", k)
    k = k.replace("transformer.norm_final_attn", "transformer.layer_norm_final_attn")
    for a, b in (("0", "upscale_conv1"), ("1", "upscale_layer_norm"), ("3", "upscale_conv2")):
        k = re.sub(rf"^output_upscaling\.{a}\.", f"{b}.", k)
    m = re.match(r"^(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.(\d)\.(\w+)$", k)
    if m:
        k = f"{m.group(1)}." + {"0": "proj_in", "1": "layers.0", "2": "proj_out"}[m.group(2)] + f".{m.group(3)}"
    return which, k


# ------------------------------------------------------------------------------------------------ the predictor's host maths
def get_preprocess_shape(oldh, oldw, long_side_length):
    scale = long_side_length * 1.0 / max(oldh, oldw)
    return int(oldh * scale + 0.5), int(oldw * scale + 0.5)


def postprocess_masks(masks, image_size0, input_size, original_size):
    masks = F.interpolate(masks, (image_size0, image_size0), mode="bilinear", align_corners=False)
    masks = masks[..., :input_size[0], :input_size[1]]
    return F.interpolate(masks, tuple(original_size), mode="bilinear", align_corners=False)


# ------------------------------------------------------------------------------------------------ the fixture's model (tests/golden/sam_golden.npz)
def seeded_oracle(gold):
    """(PromptEncoder, MaskDecoder) in fp32 with the weights the fixture was made with."""
    size = int(gold["cfg_image_size"][0])
    pe, md = build((64, 64), (size, size), mlp_dim=int(gold["cfg_mlp_dim"]))
    return seed_state(pe, int(gold["cfg_seed_pe"])), seed_state(md, int(gold["cfg_seed_md"]))


def narrow_model(gold, dtype=torch.float16, device=None):
    """omg_amd.sam.EfficientViTSam of the fixture: the narrow encoder of effvit_golden.npz, the seeded prompt encoder and decoder,
    loaded as one checkpoint-shaped state dict."""
    import os
    from omg_amd import sam
    from omg_amd.efficientvit import EfficientViTSamImageEncoder
    from tests.effvit_torch import load_fixture
    _, cfg, enc_sd, _, _ = load_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "effvit_golden.npz"))
    size = tuple(int(v) for v in gold["cfg_image_size"])
    m = sam.EfficientViTSam(EfficientViTSamImageEncoder(cfg, dtype=dtype, device=device),
                            sam.SamPromptEncoder(256, (64, 64), (size[0], size[0]), 16, dtype=dtype, device=device),
                            sam.SamMaskDecoder(256, 3, 2, 8, int(gold["cfg_mlp_dim"]), 3, 256, dtype=dtype, device=device), image_size=size)
    pe, md = seeded_oracle(gold)
    sd = {"image_encoder." + k: v for k, v in enc_sd.items()}
    sd.update({"prompt_encoder." + k: v for k, v in pe.state_dict().items()})
    sd.update({"mask_decoder." + k: v for k, v in md.state_dict().items()})
    m.load_state_dict(sd, strict=True)
    return m
