"""The Swin backbone (``transformers.SwinBackbone``, the image backbone of GroundingDINO) in plain torch fp32: the oracle of
omg_amd/swin.py.

Written literally from the published architecture — Liu et al., "Swin Transformer: Hierarchical Vision Transformer using Shifted
Windows" (2021) — as the library runs it for a backbone: the window is never clamped to the grid (``always_partition``), the grid is
zero-padded AFTER ``layernorm_before`` to a multiple of the window, rolled by ``-shift``, partitioned, attended with the table's bias
and the additive -100 region mask, reversed, rolled back and cropped.  It works on a state dict under the library's own key names, so
the dict moves between this file, ``transformers.SwinBackbone`` and ``omg_amd.SwinBackbone`` key for key; tests/test_swin.py pins it
against the library class.

``forward(sd, cfg, x, twin=dtype)`` is the 16-bit twin: every operation's output rounded to ``dtype`` (weights too), the error scale
the HIP path is held to.  ``defect=`` runs the network with one deliberate mistake; the fixture's generator asserts that each of them
moves the output by far more than the twin's rounding — a fixture that could not tell them apart would prove nothing.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.sam_torch import checksum  # noqa: F401  (re-exported)

DEFECTS = ("no_shift_mask", "pad_keys_excluded", "roll_reversed", "bias_index_flipped", "merge_order_permuted")


def small_cfg(name):
    """The two fixture configs (``image`` is the input size H x W the fixture uses)."""
    if name == "w7":
        return dict(window_size=7, embed_dim=32, num_heads=[1, 2, 4], depths=[2, 2, 2], out_features=["stage1", "stage2", "stage3"],
                    image=(90, 118))
    if name == "w12":
        return dict(window_size=12, embed_dim=96, num_heads=[3, 6], depths=[2, 2], out_features=["stage1", "stage2"], image=(104, 152))
    raise KeyError(name)


def full_cfg():
    """GroundingDINO's Swin-B (``GroundingDINO_SwinB.cfg.py``: swin_B_384_22k)."""
    return dict(window_size=12, embed_dim=128, num_heads=[4, 8, 16, 32], depths=[2, 2, 18, 2], out_features=["stage2", "stage3", "stage4"],
                image=(800, 800))


def hf_config_dict(cfg):
    """The ``config.json`` of a checkpoint with this architecture."""
    return dict(model_type="swin", image_size=224, patch_size=4, num_channels=3, embed_dim=cfg["embed_dim"], depths=list(cfg["depths"]),
                num_heads=list(cfg["num_heads"]), window_size=cfg["window_size"], mlp_ratio=4.0, qkv_bias=True, hidden_dropout_prob=0.0,
                attention_probs_dropout_prob=0.0, drop_path_rate=0.0, hidden_act="gelu", use_absolute_embeddings=False,
                layer_norm_eps=1e-5, out_features=list(cfg["out_features"]))


def to_hf_config(cfg):
    from transformers import SwinConfig
    d = hf_config_dict(cfg)
    d.pop("model_type")
    return SwinConfig(**d)


def state_shapes(cfg):
    """key -> shape, in the order of ``SwinBackbone(cfg).state_dict()``."""
    E, S = cfg["embed_dim"], cfg["window_size"]
    out = {"swin.embeddings.patch_embeddings.projection.weight": (E, 3, 4, 4), "swin.embeddings.patch_embeddings.projection.bias": (E,),
           "swin.embeddings.norm.weight": (E,), "swin.embeddings.norm.bias": (E,)}
    n = len(cfg["depths"])
    for li, (depth, heads) in enumerate(zip(cfg["depths"], cfg["num_heads"])):
        C = E << li
        for bi in range(depth):
            p = f"swin.encoder.layers.{li}.blocks.{bi}."
            for nm in ("q_proj", "k_proj", "v_proj", "o_proj"):
                out[p + f"attention.{nm}.weight"], out[p + f"attention.{nm}.bias"] = (C, C), (C,)
            out[p + "attention.relative_position_bias.relative_position_bias_table"] = ((2 * S - 1) ** 2, heads)
            for nm in ("layernorm_before", "layernorm_after"):
                out[p + nm + ".weight"], out[p + nm + ".bias"] = (C,), (C,)
            out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = (4 * C, C), (4 * C,)
            out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = (C, 4 * C), (C,)
        if li < n - 1:
            p = f"swin.encoder.layers.{li}.downsample."
            out[p + "reduction.weight"], out[p + "norm.weight"], out[p + "norm.bias"] = (2 * C, 4 * C), (4 * C,), (4 * C,)
    out["swin.layernorm.weight"], out["swin.layernorm.bias"] = (E << (n - 1),), (E << (n - 1),)       # SwinModel's; the backbone never runs it
    for st in cfg["out_features"]:
        C = E << (int(st[5:]) - 1)
        out[f"hidden_states_norms.{st}.weight"], out[f"hidden_states_norms.{st}.bias"] = (C,), (C,)
    return out


def seed_state(cfg, seed):
    """A state dict filled, in key order, from ``np.random.RandomState(seed)`` (MT19937) on the fp16 grid: matrices normal at
    1.4 / sqrt(fan_in), norm gains 1 +- 0.2, biases +- 0.1 — and the q / k projections at 1.25x that scale (q.k / sqrt(32) then has a
    standard deviation of about 3) and the bias tables at +- 1.5, so that the scores spread over several units and the softmax rows are
    far from uniform: under a near-uniform softmax a wrong mask, shift or bias index barely shows.  Much
    larger scales make the softmax an argmax and the network chaotic: the 16-bit twin itself then misses the fp32 result by tens of
    per cent and nothing can be held to it."""
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape in state_shapes(cfg).items():
        z = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
        if key.endswith("relative_position_bias_table"):
            v = 1.5 * z
        elif "norm" in key and len(shape) == 1:
            v = 1.0 + 0.2 * z if key.endswith("weight") else 0.1 * z
        elif key.endswith("bias"):
            v = 0.1 * z
        else:
            v = 1.4 * z / math.sqrt(z[0].numel())
            if ".q_proj." in key or ".k_proj." in key:
                v = 1.25 * v
        sd[key] = v.half().float()
    return sd


def seeded_input(seed, B, H, W):
    """[B, 3, H, W] as int8: pixel value = q / 8 (normal, rounded to that grid: exact in fp16 and bf16)."""
    rs = np.random.RandomState(seed)
    return np.clip(np.round(rs.standard_normal((B, 3, H, W)) * 8.0), -127, 127).astype(np.int8)


def rel_rms(a, b):
    """rms(a - b) / rms(b)."""
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


# ------------------------------------------------------------------------------------------------ the pieces, literally
def relative_position_index(S, flipped=False):
    c = torch.stack(torch.meshgrid([torch.arange(S), torch.arange(S)], indexing="ij")).flatten(1)            # 2, S S
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).contiguous()                                    # [query, key, 2]
    if flipped:
        rel = -rel
    return (rel[:, :, 0] + S - 1) * (2 * S - 1) + rel[:, :, 1] + S - 1


def partition(x, S):
    B, H, W, C = x.shape
    return x.view(B, H // S, S, W // S, S, C).transpose(2, 3).reshape(-1, S * S, C)


def reverse(w, S, H, W):
    C = w.shape[-1]
    return w.view(-1, H // S, W // S, S, S, C).transpose(2, 3).reshape(-1, H, W, C)


def shift_mask(Hp, Wp, S, shift):
    """[windows, S S (query), S S (key)]: 0 where the regions agree, -100 where they differ."""
    hi, wi = torch.arange(Hp), torch.arange(Wp)
    hr = (hi >= Hp - S).long() + (hi >= Hp - shift).long()
    wr = (wi >= Wp - S).long() + (wi >= Wp - shift).long()
    img = (hr[None, :, None, None] * 3 + wr[None, None, :, None]).float()
    mw = partition(img, S).view(-1, S * S)
    d = mw.unsqueeze(1) - mw.unsqueeze(2)
    return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))


def window_attention(y, H, W, S, shift, heads, wq, bq, wk, bk, wv, bv, table, q, defect=None):
    """``y`` [B, H W, C] after layernorm_before -> the attention output [B, H W, C] before o_proj."""
    B, _, C = y.shape
    d = C // heads
    y = y.view(B, H, W, C)
    pr, pb = (S - W % S) % S, (S - H % S) % S
    y = F.pad(y, (0, 0, 0, pr, 0, pb))
    real = F.pad(torch.ones(1, H, W, 1), (0, 0, 0, pr, 0, pb))
    Hp, Wp = H + pb, W + pr
    sgn = 1 if defect == "roll_reversed" else -1
    if shift > 0:
        y = torch.roll(y, shifts=(sgn * shift, sgn * shift), dims=(1, 2))
        real = torch.roll(real, shifts=(sgn * shift, sgn * shift), dims=(1, 2))
    win = partition(y, S)                                                                                     # [B nW, N, C]
    nW = win.shape[0] // B
    qq, kk, vv = (q(F.linear(win, w_, b_)).view(-1, S * S, heads, d).transpose(1, 2) for w_, b_ in ((wq, bq), (wk, bk), (wv, bv)))
    bias = table[relative_position_index(S, defect == "bias_index_flipped").view(-1)].view(S * S, S * S, heads).permute(2, 0, 1)
    s = qq @ kk.transpose(-1, -2) * d ** -0.5 + bias[None]
    if shift > 0 and defect != "no_shift_mask":
        s = s + shift_mask(Hp, Wp, S, shift).repeat(B, 1, 1)[:, None]
    if defect == "pad_keys_excluded":
        keep = partition(real, S).view(nW, 1, 1, S * S).repeat(B, 1, 1, 1)
        s = s.masked_fill(keep == 0, float("-inf"))
    o = q(torch.softmax(s, dim=-1) @ vv).transpose(1, 2).reshape(-1, S * S, C)
    o = reverse(o, S, Hp, Wp)
    if shift > 0:
        o = torch.roll(o, shifts=(-sgn * shift, -sgn * shift), dims=(1, 2))
    return o[:, :H, :W].reshape(B, H * W, C)


def patch_merge(t, H, W, permuted=False):
    """[B, H W, C] -> [B, ceil(H/2) ceil(W/2), 4 C] (before the norm)."""
    B, _, C = t.shape
    t = F.pad(t.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    order = [(r, c) for r in range(2) for c in range(2)] if permuted else [(r, c) for c in range(2) for r in range(2)]
    return torch.cat([t[:, r::2, c::2] for r, c in order], dim=-1).view(B, -1, 4 * C)


def forward(sd, cfg, x, twin=None, defect=None):
    """-> dict: ``embeddings`` [B, Hg Wg, E], ``stage1`` .. ``stageN`` [B, h w, C] before downsampling, ``feature_maps`` (NCHW tuple, one
    per out_feature, through its hidden_states_norms), ``grids`` [(h, w)] per stage."""
    assert defect is None or defect in DEFECTS
    if twin is None:
        q = lambda t: t                                                              # noqa: E731
    else:
        q = lambda t: t.to(twin).float()                                             # noqa: E731
    w = lambda k: q(sd[k])                                                           # noqa: E731
    S, E, eps = cfg["window_size"], cfg["embed_dim"], 1e-5

    def ln(p, t, e=eps):
        return q(F.layer_norm(t, (t.shape[-1],), w(p + ".weight"), w(p + ".bias"), e))

    x = q(x)
    B, _, Hi, Wi = x.shape
    x = F.pad(x, (0, (4 - Wi % 4) % 4, 0, (4 - Hi % 4) % 4))
    P = "swin.embeddings."
    t = q(F.conv2d(x, w(P + "patch_embeddings.projection.weight"), w(P + "patch_embeddings.projection.bias"), stride=4))
    H, W = t.shape[2:]
    t = ln(P + "norm", t.flatten(2).transpose(1, 2))
    out = {"embeddings": t, "grids": []}
    n = len(cfg["depths"])
    maps = []
    for li, (depth, heads) in enumerate(zip(cfg["depths"], cfg["num_heads"])):
        for bi in range(depth):
            p = f"swin.encoder.layers.{li}.blocks.{bi}."
            a = p + "attention."
            y = ln(p + "layernorm_before", t)
            o = window_attention(y, H, W, S, 0 if bi % 2 == 0 else S // 2, heads, w(a + "q_proj.weight"), w(a + "q_proj.bias"),
                                 w(a + "k_proj.weight"), w(a + "k_proj.bias"), w(a + "v_proj.weight"), w(a + "v_proj.bias"),
                                 w(a + "relative_position_bias.relative_position_bias_table"), q, defect)
            t = q(F.linear(o, w(a + "o_proj.weight"), w(a + "o_proj.bias")) + t)
            y = ln(p + "layernorm_after", t)
            y = q(F.gelu(q(F.linear(y, w(p + "mlp.fc1.weight"), w(p + "mlp.fc1.bias")))))
            t = q(F.linear(y, w(p + "mlp.fc2.weight"), w(p + "mlp.fc2.bias")) + t)
        out[f"stage{li + 1}"] = t
        out["grids"].append((H, W))
        if f"stage{li + 1}" in cfg["out_features"]:
            f = ln(f"hidden_states_norms.stage{li + 1}", t)
            maps.append(f.view(B, H, W, -1).permute(0, 3, 1, 2).contiguous())
        if li < n - 1:
            p = f"swin.encoder.layers.{li}.downsample."
            m = ln(p + "norm", patch_merge(t, H, W, defect == "merge_order_permuted"))
            t = q(F.linear(m, w(p + "reduction.weight")))
            H, W = (H + 1) // 2, (W + 1) // 2
    out["feature_maps"] = tuple(maps)
    return out


# ------------------------------------------------------------------------------------------------ other naming schemes (for the loader tests)
def to_hub_names(sd):
    """The library's current keys -> the names Hub checkpoints carry."""
    rep = ((".attention.q_proj.", ".attention.self.query."), (".attention.k_proj.", ".attention.self.key."),
           (".attention.v_proj.", ".attention.self.value."), (".attention.o_proj.", ".attention.output.dense."),
           (".attention.relative_position_bias.relative_position_bias_table", ".attention.self.relative_position_bias_table"),
           (".mlp.fc1.", ".intermediate.dense."), (".mlp.fc2.", ".output.dense."))
    out = {}
    for k, v in sd.items():
        for a, b in rep:
            if a in k:
                k = k.replace(a, b)
                break
        out[k] = v
    return out


def to_groundingdino_names(sd, cfg):
    """The inverse of ``omg_amd.swin.swin_from_groundingdino``: the library's keys -> the original package's ``backbone.0.*`` (q, k, v
    concatenated into ``attn.qkv``)."""
    out = {}
    for k, v in sd.items():
        if k.startswith("swin.layernorm."):
            continue
        if k.startswith("swin.embeddings.patch_embeddings.projection."):
            out["backbone.0.patch_embed.proj." + k.rsplit(".", 1)[1]] = v
        elif k.startswith("swin.embeddings.norm."):
            out["backbone.0.patch_embed.norm." + k.rsplit(".", 1)[1]] = v
        elif k.startswith("hidden_states_norms.stage"):
            st, leaf = k.split(".")[1:]
            out[f"backbone.0.norm{int(st[5:]) - 1}.{leaf}"] = v
        else:
            parts = k.split(".")                     # swin encoder layers L ...
            L = parts[3]
            rest = ".".join(parts[4:])
            base = f"backbone.0.layers.{L}."
            if rest.startswith("downsample."):
                out[base + rest] = v
                continue
            Bi = parts[5]
            leaf = ".".join(parts[6:])
            b = base + f"blocks.{Bi}."
            if leaf.startswith("attention.q_proj."):
                kind = leaf.rsplit(".", 1)[1]
                pre = f"swin.encoder.layers.{L}.blocks.{Bi}.attention."
                out[b + "attn.qkv." + kind] = torch.cat([sd[pre + f"{n}_proj.{kind}"] for n in "qkv"], dim=0)
            elif leaf.startswith("attention.k_proj.") or leaf.startswith("attention.v_proj."):
                continue
            elif leaf.startswith("attention.o_proj."):
                out[b + "attn.proj." + leaf.rsplit(".", 1)[1]] = v
            elif leaf.startswith("attention.relative_position_bias."):
                out[b + "attn.relative_position_bias_table"] = v
            elif leaf.startswith("layernorm_before."):
                out[b + "norm1." + leaf.rsplit(".", 1)[1]] = v
            elif leaf.startswith("layernorm_after."):
                out[b + "norm2." + leaf.rsplit(".", 1)[1]] = v
            else:
                out[b + leaf] = v                    # mlp.fc1 / mlp.fc2
    return out


# ------------------------------------------------------------------------------------------------ the attention alone, from fused QKV rows
def attention_from_qkv(qkv, B, H, W, heads, S, shift, table, pad_kv=None, scale=None, p_round=None):
    """What omg_attn_swin computes, literally (pad, roll, partition, bias, mask, softmax, reverse, roll back, crop), in the dtype of
    ``qkv`` [B H W, 3 heads d] (float64 for a reference) -> [B H W, heads d].  A padded position is a key with k | v = ``pad_kv``
    [2 heads d] (None: zeros).  ``p_round``: the storage dtype of the rounding model — probabilities relative to the row maximum
    rounded to it before P V, the row sum taken on the unrounded ones — else the plain softmax."""
    C = qkv.shape[1] // 3
    d = C // heads
    scale = d ** -0.5 if scale is None else scale
    t = qkv.view(B, H, W, 3 * C)
    pr, pb = (S - W % S) % S, (S - H % S) % S
    Hp, Wp = H + pb, W + pr
    full = torch.zeros(B, Hp, Wp, 3 * C, dtype=qkv.dtype)
    if pad_kv is not None:
        full[..., C:] = pad_kv.to(qkv.dtype)
    full[:, :H, :W] = t
    if shift > 0:
        full = torch.roll(full, shifts=(-shift, -shift), dims=(1, 2))
    win = partition(full, S)
    q, k, v = (win[..., i * C:(i + 1) * C].reshape(-1, S * S, heads, d).transpose(1, 2) for i in range(3))
    bias = table.to(qkv.dtype)[relative_position_index(S).view(-1)].view(S * S, S * S, heads).permute(2, 0, 1)
    s = q @ k.transpose(-1, -2) * scale + bias[None]
    if shift > 0:
        s = s + shift_mask(Hp, Wp, S, shift).to(qkv.dtype).repeat(B, 1, 1)[:, None]
    if p_round is None:
        o = torch.softmax(s, dim=-1) @ v
    else:
        e = torch.exp(s - s.amax(dim=-1, keepdim=True))
        o = (e.to(p_round).to(qkv.dtype) @ v) / e.sum(dim=-1, keepdim=True)
    o = reverse(o.transpose(1, 2).reshape(-1, S * S, C), S, Hp, Wp)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o[:, :H, :W].reshape(B * H * W, C)


def region_of(H, W, S, shift):
    """[H, W] long: the shift region (0 .. 8) of every position of the UNPADDED grid (the padded grid rolled by -shift carries
    ``shift_mask``'s regions; this is where each image position ends up)."""
    Hp, Wp = -(-H // S) * S, -(-W // S) * S
    hi, wi = torch.arange(Hp), torch.arange(Wp)
    hr = (hi >= Hp - S).long() + (hi >= Hp - shift).long()
    wr = (wi >= Wp - S).long() + (wi >= Wp - shift).long()
    img = hr[:, None] * 3 + wr[None, :]                               # regions of the ROLLED grid
    return torch.roll(img, shifts=(shift, shift), dims=(0, 1))[:H, :W]
