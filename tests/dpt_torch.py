"""The DPT-hybrid depth estimator (``dpt-hybrid-midas``) in plain torch fp32: the oracle of omg_amd/dpt.py.

Written from the published architecture — Ranftl et al., "Vision Transformers for Dense Prediction" (2021): a BiT ResNet-50 stem and
three stages (Kolesnikov et al., "Big Transfer", 2020: weight-standardised convolutions, GroupNorm, TF-"SAME" padding) feeding a ViT,
the reassemble / fusion neck and the three-convolution head — under the parameter names of the Hugging Face checkpoint, so that a state
dict moves between this module, ``transformers.DPTForDepthEstimation`` and ``omg_amd.DPTForDepthEstimation`` key for key.
tests/test_dpt.py pins it against the library class.

``cfg`` is a plain dict (``small_cfg`` / ``full_cfg``); ``to_hf_config`` makes the library's ``DPTConfig`` of it.  ``forward(x, twin=dtype)``
is the 16-bit twin: the same network with every operation's output rounded to ``dtype`` (weights rounded too), the error scale the
HIP path is held to.  ``trace`` receives the intermediates the fixture records (all NCHW / [B, N, C] as the library has them).
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.sam_torch import checksum  # noqa: F401  (re-exported)


def small_cfg(image_size):
    """The two fixture configs: 96 (37 tokens) and 192 (145 tokens)."""
    g = image_size // 16
    return dict(image_size=image_size, patch_size=16, hidden_size=128, num_attention_heads=2, num_hidden_layers=4, intermediate_size=512,
                layer_norm_eps=1e-12, backbone_out_indices=[0, 1, 2, 3], neck_hidden_sizes=[64, 128, 128, 128], fusion_hidden_size=64,
                reassemble_factors=[1, 1, 1, 0.5], backbone_featmap_shape=[1, 256, g, g],
                bit=dict(depths=[2, 1, 2], hidden_sizes=[64, 128, 256], embedding_size=32, num_groups=8))


def full_cfg():
    """``Intel/dpt-hybrid-midas``."""
    return dict(image_size=384, patch_size=16, hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072,
                layer_norm_eps=1e-12, backbone_out_indices=[2, 5, 8, 11], neck_hidden_sizes=[256, 512, 768, 768], fusion_hidden_size=256,
                reassemble_factors=[1, 1, 1, 0.5], backbone_featmap_shape=[1, 1024, 24, 24],
                bit=dict(depths=[3, 4, 9], hidden_sizes=[256, 512, 1024], embedding_size=64, num_groups=32))


def hf_config_dict(cfg):
    """The ``config.json`` of a checkpoint with this architecture (what ``to_hf_config`` builds, as a dict)."""
    b = cfg["bit"]
    d = {k: cfg[k] for k in ("image_size", "patch_size", "hidden_size", "num_attention_heads", "num_hidden_layers", "intermediate_size",
                             "layer_norm_eps", "backbone_out_indices", "neck_hidden_sizes", "fusion_hidden_size", "reassemble_factors",
                             "backbone_featmap_shape")}
    d.update(model_type="dpt", is_hybrid=True, hidden_act="gelu", qkv_bias=True, readout_type="project", num_channels=3,
             neck_ignore_stages=[0, 1], use_batch_norm_in_fusion_residual=False, use_bias_in_fusion_residual=True, add_projection=False,
             head_in_index=-1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
             backbone_config=dict(model_type="bit", depths=b["depths"], hidden_sizes=b["hidden_sizes"], embedding_size=b["embedding_size"],
                                  num_groups=b["num_groups"], layer_type="bottleneck", global_padding="same", embedding_dynamic_padding=True,
                                  hidden_act="relu", num_channels=3, out_features=["stage1", "stage2", "stage3"]))
    return d


def to_hf_config(cfg):
    from transformers import DPTConfig
    d = hf_config_dict(cfg)
    d.pop("model_type")
    return DPTConfig(**d)


# ------------------------------------------------------------------------------------------------ building blocks
def same_pad(x, k, stride, value=0.0):
    """TF "SAME": total padding p per axis, p // 2 in front and the rest behind."""
    H, W = x.shape[-2:]
    ph = max((math.ceil(H / stride) - 1) * stride + k - H, 0)
    pw = max((math.ceil(W / stride) - 1) * stride + k - W, 0)
    return F.pad(x, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2], value=value) if ph or pw else x


def standardize(w, eps=1e-8):
    """Weight standardisation: per output channel (w - mean) / sqrt(biased var + eps)."""
    m = w.mean(dim=(1, 2, 3), keepdim=True)
    v = w.var(dim=(1, 2, 3), keepdim=True, unbiased=False)
    return (w - m) / torch.sqrt(v + eps)


class WSConv(nn.Module):
    def __init__(self, cin, cout, k, stride=1):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, k, k))
        self.k, self.stride = k, stride


class GN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.ones(c)), nn.Parameter(torch.zeros(c))


class Downsample(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv, self.norm = WSConv(cin, cout, 1, stride), GN(cout)


class Bottleneck(nn.Module):
    def __init__(self, cin, cout, stride, first):
        super().__init__()
        mid = cout // 4
        if first:
            self.downsample = Downsample(cin, cout, stride)
        self.conv1, self.norm1 = WSConv(cin, mid, 1), GN(mid)
        self.conv2, self.norm2 = WSConv(mid, mid, 3, stride), GN(mid)
        self.conv3, self.norm3 = WSConv(mid, cout, 1), GN(cout)


class Stage(nn.Module):
    def __init__(self, cin, cout, stride, depth):
        super().__init__()
        self.layers = nn.ModuleList([Bottleneck(cin if i == 0 else cout, cout, stride if i == 0 else 1, i == 0) for i in range(depth)])


class Embedder(nn.Module):
    def __init__(self, e):
        super().__init__()
        self.convolution, self.norm = WSConv(3, e, 7, 2), GN(e)


class BitEncoder(nn.Module):
    def __init__(self, b):
        super().__init__()
        chans = [b["embedding_size"]] + list(b["hidden_sizes"])
        self.stages = nn.ModuleList([Stage(chans[i], chans[i + 1], 1 if i == 0 else 2, d) for i, d in enumerate(b["depths"])])


class Bit(nn.Module):
    def __init__(self, b):
        super().__init__()
        self.embedder, self.encoder = Embedder(b["embedding_size"]), BitEncoder(b)


class Backbone(nn.Module):
    def __init__(self, b):
        super().__init__()
        self.bit = Bit(b)


class Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        D, n = cfg["hidden_size"], (cfg["image_size"] // cfg["patch_size"]) ** 2
        self.cls_token = nn.Parameter(torch.zeros(1, 1, D))
        self.position_embeddings = nn.Parameter(torch.zeros(1, n + 1, D))
        self.backbone = Backbone(cfg["bit"])
        self.projection = nn.Conv2d(cfg["backbone_featmap_shape"][1], D, 1)


class SelfAttention(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(D, D), nn.Linear(D, D), nn.Linear(D, D)


class Dense(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.dense = nn.Linear(i, o)


class Attention(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.attention, self.output = SelfAttention(D), Dense(D, D)


class Layer(nn.Module):
    def __init__(self, D, I, eps):
        super().__init__()
        self.attention, self.intermediate, self.output = Attention(D), Dense(D, I), Dense(I, D)
        self.layernorm_before, self.layernorm_after = nn.LayerNorm(D, eps=eps), nn.LayerNorm(D, eps=eps)


class Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([Layer(cfg["hidden_size"], cfg["intermediate_size"], cfg["layer_norm_eps"]) for _ in range(cfg["num_hidden_layers"])])


class DPTModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings, self.encoder = Embeddings(cfg), Encoder(cfg)
        self.layernorm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])       # in the checkpoint, never on the depth path


class Reassemble(nn.Module):
    def __init__(self, D, c, factor):
        super().__init__()
        self.projection = nn.Conv2d(D, c, 1)
        if factor < 1:
            self.resize = nn.Conv2d(c, c, 3, stride=int(1 / factor), padding=1)


class ReassembleStage(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        D = cfg["hidden_size"]
        self.layers = nn.ModuleList([nn.Identity() if i < 2 else Reassemble(D, c, f)
                                     for i, (c, f) in enumerate(zip(cfg["neck_hidden_sizes"], cfg["reassemble_factors"]))])
        self.readout_projects = nn.ModuleList([nn.Sequential(nn.Identity()) if i < 2 else nn.Sequential(nn.Linear(2 * D, D), nn.GELU())
                                               for i in range(len(cfg["neck_hidden_sizes"]))])


class ResidualUnit(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.convolution1, self.convolution2 = nn.Conv2d(c, c, 3, padding=1), nn.Conv2d(c, c, 3, padding=1)


class Fusion(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.projection = nn.Conv2d(c, c, 1)
        self.residual_layer1, self.residual_layer2 = ResidualUnit(c), ResidualUnit(c)


class FusionStage(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([Fusion(cfg["fusion_hidden_size"]) for _ in cfg["neck_hidden_sizes"]])


class Neck(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.reassemble_stage = ReassembleStage(cfg)
        self.convs = nn.ModuleList([nn.Conv2d(c, cfg["fusion_hidden_size"], 3, padding=1, bias=False) for c in cfg["neck_hidden_sizes"]])
        self.fusion_stage = FusionStage(cfg)


class Head(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.head = nn.Sequential(nn.Conv2d(c, c // 2, 3, padding=1), nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True),
                                  nn.Conv2d(c // 2, 32, 3, padding=1), nn.ReLU(), nn.Conv2d(32, 1, 1), nn.ReLU())


class DPTHybrid(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.dpt, self.neck, self.head = DPTModel(cfg), Neck(cfg), Head(cfg["fusion_hidden_size"])
        self.trace = None

    # -------------------------------------------------------------------------------------------- forward
    def forward(self, x, twin=None):
        cfg = self.cfg
        if twin is None:
            q = lambda t: t                                                          # noqa: E731
        else:
            q = lambda t: t.to(twin).float()                                         # noqa: E731
        tr = self.trace if self.trace is not None else {}
        G = cfg["bit"]["num_groups"]

        def wsconv(m, t):
            w = q(standardize(m.weight))                       # folded in fp32, rounded once (what the HIP module stores)
            return q(F.conv2d(same_pad(t, m.k, m.stride) if m.stride > 1 else t, w, None, m.stride, 0 if m.stride > 1 else m.k // 2))

        def gn(m, t, relu=True, res=None):
            y = q(F.group_norm(t, G, q(m.weight), q(m.bias), 1e-5))
            if res is not None:
                y = q(y + res)
            return q(F.relu(y)) if relu else y

        def conv(m, t, **kw):
            return q(F.conv2d(t, q(m.weight), None if m.bias is None else q(m.bias), **kw))

        def lin(m, t):
            return q(F.linear(t, q(m.weight), q(m.bias)))

        def up2(t):
            return q(F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True))

        x = q(x)
        bit = self.dpt.embeddings.backbone.bit
        h = gn(bit.embedder.norm, wsconv(bit.embedder.convolution, x))
        h = F.max_pool2d(same_pad(h, 3, 2), 3, 2)
        maps = []
        for st in bit.encoder.stages:
            for blk in st.layers:
                sc = gn(blk.downsample.norm, wsconv(blk.downsample.conv, h), relu=False) if hasattr(blk, "downsample") else h
                t = gn(blk.norm1, wsconv(blk.conv1, h))
                t = gn(blk.norm2, wsconv(blk.conv2, t))
                h = gn(blk.norm3, wsconv(blk.conv3, t), relu=True, res=sc)
            maps.append(h)
        tr["bit_stage1"], tr["bit_stage2"] = maps[0], maps[1]

        emb = self.dpt.embeddings
        t = conv(emb.projection, maps[2]).flatten(2).transpose(1, 2)
        B, N, D = t.shape
        t = q(torch.cat([q(emb.cls_token).expand(B, -1, -1), t], dim=1) + q(emb.position_embeddings))
        nh = cfg["num_attention_heads"]
        taps = []
        for i, ly in enumerate(self.dpt.encoder.layer):
            y = q(F.layer_norm(t, (D,), q(ly.layernorm_before.weight), q(ly.layernorm_before.bias), cfg["layer_norm_eps"]))
            a = ly.attention.attention
            qq, kk, vv = (lin(m, y).view(B, N + 1, nh, D // nh).transpose(1, 2) for m in (a.query, a.key, a.value))
            o = q(torch.softmax(qq @ kk.transpose(-1, -2) * (D // nh) ** -0.5, dim=-1) @ vv)
            t = q(lin(ly.attention.output.dense, o.transpose(1, 2).reshape(B, N + 1, D)) + t)
            y = q(F.layer_norm(t, (D,), q(ly.layernorm_after.weight), q(ly.layernorm_after.bias), cfg["layer_norm_eps"]))
            t = q(lin(ly.output.dense, q(F.gelu(lin(ly.intermediate.dense, y)))) + t)
            if i in cfg["backbone_out_indices"][2:]:
                taps.append(t)
        tr["vit_tap0"], tr["vit_tap1"] = taps

        rs = self.neck.reassemble_stage
        g = int(round(math.sqrt(N)))
        feats = [maps[0], maps[1]]
        for i, hs in zip((2, 3), taps):
            cls, tok = hs[:, :1], hs[:, 1:]
            z = q(F.gelu(lin(rs.readout_projects[i][0], torch.cat([tok, cls.expand_as(tok)], dim=-1))))
            z = z.transpose(1, 2).reshape(B, D, g, g)
            z = conv(rs.layers[i].projection, z)
            if hasattr(rs.layers[i], "resize"):
                z = conv(rs.layers[i].resize, z, stride=2, padding=1)
            feats.append(z)
        feats = [conv(m, f, padding=1) for m, f in zip(self.neck.convs, feats)]

        def unit(m, t):
            u = conv(m.convolution1, q(F.relu(t)), padding=1)
            return q(conv(m.convolution2, q(F.relu(u)), padding=1) + t)

        fused = None
        for i, (f, ly) in enumerate(zip(feats[::-1], self.neck.fusion_stage.layers)):
            if fused is None:
                fused = f
            else:
                assert fused.shape == f.shape
                fused = q(fused + unit(ly.residual_layer1, f))
            fused = conv(ly.projection, up2(unit(ly.residual_layer2, fused)))
            tr[f"fused{i}"] = fused
        hd = self.head.head
        t = up2(conv(hd[0], fused, padding=1))
        t = q(F.relu(conv(hd[2], t, padding=1)))
        return F.relu(F.conv2d(t, q(hd[4].weight), q(hd[4].bias)))[:, 0]             # fp32 out, as the HIP head writes it


# ------------------------------------------------------------------------------------------------ seeding
def seed_state(module, seed):
    """Fill every parameter, in state-dict order, from ``np.random.RandomState(seed)`` (MT19937) on the fp16 grid.  The library's default
    initialisation leaves the final ReLU dead (98 % exact zeros on a small config), so: matrices and convolutions normal at
    1.4 / sqrt(fan_in), norm gains 1 +- 0.2, biases +- 0.1, tokens and positions at 0.5, the last bias positive and the last projection's weights shifted by one standard deviation towards the
    positive side (its inputs are ReLU outputs: the depth is then positive almost everywhere, and the final ReLU still clips a little)."""
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for key, t in module.state_dict().items():
            z = torch.from_numpy(rs.standard_normal(tuple(t.shape)).astype(np.float32))
            if key == "head.head.4.bias":
                v = 0.5 + 0.1 * z.abs()
            elif key == "head.head.4.weight":
                v = 1.4 * (z + 1.0) / math.sqrt(t[0].numel())
            elif "norm" in key and t.dim() == 1:
                v = 1.0 + 0.2 * z if key.endswith("weight") else 0.1 * z
            elif key.endswith("bias"):
                v = 0.1 * z
            elif key.endswith("cls_token") or key.endswith("position_embeddings"):
                v = 0.5 * z
            else:
                v = 1.4 * z / math.sqrt(t[0].numel())
            t.copy_(v.half().float())
    return module


def seeded_input(seed, B, size):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((B, 3, size, size)).astype(np.float32)).half().float()


def rel_rms(a, b):
    """rms(a - b) / rms(b)."""
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
