"""GroundingDINO's neck and feature enhancer (transformers' GroundingDinoModel.input_proj_vision / level_embed / text_projection and
GroundingDinoEncoder) in plain fp32 torch, written literally: grid_sample, masked_fill, the shifts and clamps of the bi-attention, the
additive finfo.min mask of the text self-attention.  The oracle of omg_amd/gdino.py (tests/test_gdino.py pins it to the live library
classes; tests/test_gdino_gpu.py holds the HIP module to it).

`forward(sd, cfg, ...)` takes the library's state-dict keys without a prefix.  `twin=dtype` rounds every operation's result to the
16-bit type (the weights are expected rounded by the caller): the yardstick of what 16-bit storage costs on a given input.  `defect=`
names one deliberate mistake (tests/golden/make_golden_gdino.py proves that the fixture sees each of them).

Masks, as the library's GroundingDinoModel.forward makes them: pixel_mask [B, H, W] 1 = valid, text_token_mask [B, T] True = a real
token, text_self_attention_masks [B, T, T] True = attend (generate_masks_with_special_tokens_and_transfer_map), position_ids [B, T].
"""
import math

import torch
import torch.nn.functional as F

DEFECTS = ("align_corners", "no_value_mask", "swap_normalizer", "valid_ratio_one", "no_vision_key_mask", "no_text_key_mask",
           "no_text_self_mask", "no_text_pos", "residual_unnormed")

_BASE = dict(d_model=256, encoder_attention_heads=8, encoder_ffn_dim=2048, encoder_n_points=4, num_feature_levels=4, encoder_layers=2,
             activation_function="relu", position_embedding_type="sine", positional_embedding_temperature=20, layer_norm_eps=1e-5,
             max_text_len=256, text_hidden=96, in_channels=[64, 128, 256])

_SMALL = {
    # B = 2; sample 1's pixel mask pads its right and bottom; T = 11: [CLS] p p . p p p . p [SEP] pad-ish, two padded tokens in sample 0
    "a": dict(grids=[(13, 19), (7, 10), (4, 5)], image=(104, 152), B=2, T=11, phrases=[(1, 3), (4, 7), (8, 9)], padded=[2, 0], pixel_pad=True),
    # no pixel mask; T = 37, one phrase of 30 tokens
    "b": dict(grids=[(9, 25), (5, 13), (3, 7)], image=(72, 200), B=2, T=37, phrases=[(1, 31), (32, 35)], padded=[0, 0], pixel_pad=False),
}


def small_cfg(name: str) -> dict:
    c = dict(_BASE)
    c.update(_SMALL[name])
    c["name"] = name
    return c


def rel_rms(x: torch.Tensor, ref: torch.Tensor) -> float:
    return math.sqrt(float(((x.double() - ref.double()) ** 2).mean()) / max(float((ref.double() ** 2).mean()), 1e-60))


def shapes(cfg: dict) -> dict:
    d, ffn, H8, L, P = cfg["d_model"], cfg["encoder_ffn_dim"], cfg["encoder_attention_heads"], cfg["num_feature_levels"], cfg["encoder_n_points"]
    E = ffn // 2
    out = {"level_embed": (L, d), "text_projection.weight": (d, cfg["text_hidden"]), "text_projection.bias": (d,)}
    cin = cfg["in_channels"]
    for l in range(L):
        k = 1 if l < len(cin) else 3
        ci = cin[l] if l < len(cin) else (cin[-1] if l == len(cin) else d)
        out[f"input_proj_vision.{l}.0.weight"], out[f"input_proj_vision.{l}.0.bias"] = (d, ci, k, k), (d,)
        out[f"input_proj_vision.{l}.1.weight"], out[f"input_proj_vision.{l}.1.bias"] = (d,), (d,)
    for i in range(cfg["encoder_layers"]):
        p = f"encoder.layers.{i}."
        f = p + "fusion_layer."
        out[f + "vision_param"], out[f + "text_param"] = (d,), (d,)
        for n in ("layer_norm_vision", "layer_norm_text"):
            out[f + n + ".weight"], out[f + n + ".bias"] = (d,), (d,)
        for n in ("vision_proj", "text_proj", "values_vision_proj", "values_text_proj"):
            out[f + f"attn.{n}.weight"], out[f + f"attn.{n}.bias"] = (E, d), (E,)
        for n in ("out_vision_proj", "out_text_proj"):
            out[f + f"attn.{n}.weight"], out[f + f"attn.{n}.bias"] = (d, E), (d,)
        t = p + "text_enhancer_layer."
        for n in ("query", "key", "value", "out_proj"):
            out[t + f"self_attn.{n}.weight"], out[t + f"self_attn.{n}.bias"] = (d, d), (d,)
        out[t + "fc1.weight"], out[t + "fc1.bias"], out[t + "fc2.weight"], out[t + "fc2.bias"] = (E, d), (E,), (d, E), (d,)
        for n in ("layer_norm_before", "layer_norm_after"):
            out[t + n + ".weight"], out[t + n + ".bias"] = (d,), (d,)
        m = p + "deformable_layer."
        out[m + "self_attn.sampling_offsets.weight"], out[m + "self_attn.sampling_offsets.bias"] = (H8 * L * P * 2, d), (H8 * L * P * 2,)
        out[m + "self_attn.attention_weights.weight"], out[m + "self_attn.attention_weights.bias"] = (H8 * L * P, d), (H8 * L * P,)
        for n in ("value_proj", "output_proj"):
            out[m + f"self_attn.{n}.weight"], out[m + f"self_attn.{n}.bias"] = (d, d), (d,)
        out[m + "fc1.weight"], out[m + "fc1.bias"], out[m + "fc2.weight"], out[m + "fc2.bias"] = (ffn, d), (ffn,), (d, ffn), (d,)
        for n in ("self_attn_layer_norm", "final_layer_norm"):
            out[m + n + ".weight"], out[m + n + ".bias"] = (d,), (d,)
    return out


def seed_state(cfg: dict, seed: int) -> dict:
    """Seeded weights under which nothing of the enhancer vanishes: Linear weights N(0, g^2 / fan_in) with gains that leave every softmax
    far from uniform, layer scales (vision_param / text_param) of order 1 instead of the library's 1e-4, offsets of a few pixels (the
    library's initialisation is near zero) that leave the smaller levels for part of the queries, norm weights around 1."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes(cfg).items():
        if k.endswith("_param"):
            v = 0.6 + 0.8 * torch.rand(s, generator=g)
        elif k == "level_embed":
            v = torch.randn(s, generator=g)
        elif ".1.weight" in k or "norm" in k and k.endswith(".weight"):
            v = 1.0 + 0.2 * torch.randn(s, generator=g)
        elif k.endswith(".bias"):
            v = 0.1 * torch.randn(s, generator=g)
            if "sampling_offsets" in k:
                v = 1.5 * torch.randn(s, generator=g)
        else:
            fan_in = 1
            for n in s[1:]:
                fan_in *= n
            gain = 1.0
            if "sampling_offsets" in k:
                gain = 2.0
            elif "attention_weights" in k:
                gain = 2.0
            elif "vision_proj" in k and "values" not in k and "out_" not in k or "text_proj." in k and "values" not in k and "out_" not in k:
                gain = 2.5                        # bi-attention q and k: scores with a standard deviation of a few units
            elif "self_attn.query" in k or "self_attn.key" in k:
                gain = 2.0
            v = torch.randn(s, generator=g) * gain / math.sqrt(fan_in)
        sd[k] = v
    return sd


def seeded_inputs(cfg: dict, seed: int) -> dict:
    """Feature maps, hidden states of the text backbone (both on the grid of eighths) and the masks of `cfg`."""
    g = torch.Generator().manual_seed(seed)
    B, T = cfg["B"], cfg["T"]
    q8 = lambda t: torch.round(t * 8.0) / 8.0
    fms = [q8(torch.randn(B, c, h, w, generator=g)) for c, (h, w) in zip(cfg["in_channels"], cfg["grids"])]
    Hi, Wi = cfg["image"]
    pixel_mask = None
    if cfg["pixel_pad"]:
        pixel_mask = torch.ones(B, Hi, Wi, dtype=torch.long)
        pixel_mask[1, int(Hi * 0.62):, :] = 0
        pixel_mask[1, :, int(Wi * 0.55):] = 0
    text = q8(torch.randn(B, T, cfg["text_hidden"], generator=g))
    token_mask = torch.ones(B, T, dtype=torch.bool)
    for b, n in enumerate(cfg["padded"]):
        if n:
            token_mask[b, T - n:] = False
    # the block mask and the position ids of generate_masks_with_special_tokens_and_transfer_map: special tokens see themselves and
    # restart the count, a phrase sees itself
    self_mask = torch.eye(T, dtype=torch.bool)[None].repeat(B, 1, 1)
    pos = torch.zeros(B, T, dtype=torch.long)
    for s, e in cfg["phrases"]:
        self_mask[:, s:e, s:e] = True
        pos[:, s:e] = torch.arange(e - s)
    return dict(feature_maps=fms, pixel_mask=pixel_mask, text_hidden_states=text, text_token_mask=token_mask,
                text_self_attention_masks=self_mask, position_ids=pos)


# ------------------------------------------------------------------ the pieces
def sine_position(mask: torch.Tensor, d_model: int, temperature: float) -> torch.Tensor:
    """GroundingDinoSinePositionEmbedding on a [B, H, W] validity mask -> [B, d_model, H, W]: y before x."""
    nd = d_model // 2
    y = mask.cumsum(1, dtype=torch.float32)
    x = mask.cumsum(2, dtype=torch.float32)
    y = y / (y[:, -1:, :] + 1e-6) * (2 * math.pi)
    x = x / (x[:, :, -1:] + 1e-6) * (2 * math.pi)
    dim_t = torch.arange(nd, dtype=torch.float32, device=mask.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / nd)
    px, py = x[:, :, :, None] / dim_t, y[:, :, :, None] / dim_t
    px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), dim=4).flatten(3)
    py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), dim=4).flatten(3)
    return torch.cat((py, px), dim=3).permute(0, 3, 1, 2)


def text_position(position_ids: torch.Tensor, d_model: int) -> torch.Tensor:
    """encode_sinusoidal_position_embedding(position_ids[..., None], d_model): one coordinate, temperature 10000."""
    dim_t = torch.arange(d_model, dtype=torch.float32, device=position_ids.device)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / d_model)
    e = position_ids[..., None] * (2 * math.pi) / dim_t          # integer ids: promoted to float32, as the library's
    # the library casts the result to the dtype of its input: with the integer ids GroundingDinoModel.forward passes, the embedding is
    # TRUNCATED to integers (1 where a cosine is exactly 1: every odd channel of id 0, channel 1 of every id; 0 elsewhere)
    return torch.stack((e[..., 0::2].sin(), e[..., 1::2].cos()), dim=-1).flatten(-2).to(position_ids.dtype)


def valid_ratio(mask: torch.Tensor) -> torch.Tensor:
    _, h, w = mask.shape
    return torch.stack([mask[:, 0, :].sum(1).float() / w, mask[:, :, 0].sum(1).float() / h], -1)


def reference_points(spatial, valid_ratios, defect=None):
    vr = torch.ones_like(valid_ratios) if defect == "valid_ratio_one" else valid_ratios
    refs = []
    for l, (h, w) in enumerate(spatial):
        ry, rx = torch.meshgrid(torch.linspace(0.5, h - 0.5, h, dtype=torch.float32, device=vr.device),
                                torch.linspace(0.5, w - 0.5, w, dtype=torch.float32, device=vr.device), indexing="ij")
        ry = ry.reshape(-1)[None] / (vr[:, None, l, 1] * h)
        rx = rx.reshape(-1)[None] / (vr[:, None, l, 0] * w)
        refs.append(torch.stack((rx, ry), -1))
    return torch.cat(refs, 1)[:, :, None] * vr[:, None]


def neck(sd, cfg, feature_maps, pixel_mask, r):
    """-> (sources [B, N, d], mask_flatten [B, N] True = valid, pos [B, N, d] with the level embedding, spatial [(h, w)], valid_ratios)."""
    B = feature_maps[0].shape[0]
    d, L = cfg["d_model"], cfg["num_feature_levels"]
    maps = []
    for l in range(L):
        w, b = sd[f"input_proj_vision.{l}.0.weight"], sd[f"input_proj_vision.{l}.0.bias"]
        if l < len(feature_maps):
            x = F.conv2d(feature_maps[l], w, b)
        else:
            # the first extra level is the convolution of the backbone's LAST feature map, later ones of the previous projected map
            x = F.conv2d(feature_maps[-1] if l == len(feature_maps) else maps[-1], w, b, stride=2, padding=1)
        x = r(x)
        maps.append(r(F.group_norm(x, 32, sd[f"input_proj_vision.{l}.1.weight"], sd[f"input_proj_vision.{l}.1.bias"], 1e-5)))
    if pixel_mask is None:
        raise ValueError("pixel_mask: pass ones for no padding (the size of the image is needed for nothing else)")
    masks = [F.interpolate(pixel_mask[None].float(), size=m.shape[-2:]).to(torch.bool)[0] for m in maps]
    src, mf, pos, spatial = [], [], [], []
    for l, (m, mk) in enumerate(zip(maps, masks)):
        spatial.append((m.shape[2], m.shape[3]))
        src.append(m.flatten(2).transpose(1, 2))
        mf.append(mk.flatten(1))
        pe = sine_position(mk, d, cfg["positional_embedding_temperature"]).flatten(2).transpose(1, 2)
        pos.append(r(pe + sd["level_embed"][l].view(1, 1, -1)))
    vr = torch.stack([valid_ratio(m) for m in masks], 1).float()
    return torch.cat(src, 1), torch.cat(mf, 1), torch.cat(pos, 1), spatial, vr, maps


def lin(sd, name, x, r):
    return r(F.linear(x, sd[name + ".weight"], sd[name + ".bias"]))


def ln(sd, name, x, eps, r):
    return r(F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps))


def bi_attention(sd, p, v, t, vision_pad, text_pad, heads, r, defect=None):
    """GroundingDinoBiMultiHeadAttention: v [B, N, d], t [B, T, d]; *_pad True = padding.  -> (delta_v, delta_t)."""
    B, N, _ = v.shape
    E = sd[p + "vision_proj.weight"].shape[0]
    hd = E // heads
    scale = hd ** -0.5
    sh = lambda x: x.view(B, -1, heads, hd).transpose(1, 2).reshape(B * heads, -1, hd)
    q = sh(r(lin(sd, p + "vision_proj", v, r) * scale))
    k = sh(lin(sd, p + "text_proj", t, r))
    vv = sh(lin(sd, p + "values_vision_proj", v, r))
    tv = sh(lin(sd, p + "values_text_proj", t, r))
    a = torch.bmm(q, k.transpose(1, 2))
    a = a - a.max()
    a = torch.clamp(a, min=-50000, max=50000)
    at = a.transpose(1, 2)
    ta = at - torch.max(at, dim=-1, keepdim=True)[0]
    ta = torch.clamp(ta, min=-50000, max=50000)
    if vision_pad is not None and defect != "no_vision_key_mask":
        ta = ta.masked_fill(vision_pad[:, None, None, :].repeat(1, heads, 1, 1).flatten(0, 1), float("-inf"))
    ta = r(ta.softmax(dim=-1))
    if text_pad is not None and defect != "no_text_key_mask":
        a = a.masked_fill(text_pad[:, None, None, :].repeat(1, heads, 1, 1).flatten(0, 1), float("-inf"))
    va = r(a.softmax(dim=-1))
    ov = r(torch.bmm(va, tv)).view(B, heads, N, hd).transpose(1, 2).reshape(B, N, E)
    ot = r(torch.bmm(ta, vv)).view(B, heads, -1, hd).transpose(1, 2).reshape(B, -1, E)
    return lin(sd, p + "out_vision_proj", ov, r), lin(sd, p + "out_text_proj", ot, r)


def text_enhancer(sd, p, h, self_mask, pos, heads, ffn, eps, r, defect=None):
    B, T, d = h.shape
    hd = d // heads
    qk = h if (pos is None or defect == "no_text_pos") else r(h + pos)
    sh = lambda x: x.view(B, T, heads, hd).transpose(1, 2)
    q, k, v = sh(lin(sd, p + "self_attn.query", qk, r)), sh(lin(sd, p + "self_attn.key", qk, r)), sh(lin(sd, p + "self_attn.value", h, r))
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    if defect != "no_text_self_mask":
        s = s + (1.0 - self_mask[:, None].float()) * torch.finfo(torch.float32).min
    a = r(F.softmax(s, dim=-1))
    o = r(torch.matmul(a, v)).permute(0, 2, 1, 3).reshape(B, T, d)
    h = ln(sd, p + "layer_norm_before", r(h + lin(sd, p + "self_attn.out_proj", o, r)), eps, r)
    y = lin(sd, p + "fc2", r(F.relu(lin(sd, p + "fc1", h, r))), r)
    return ln(sd, p + "layer_norm_after", r(y + h), eps, r)


def msdeform(sd, p, h, pos, valid, ref, spatial, heads, points, r, defect=None):
    """GroundingDinoMultiscaleDeformableAttention with the library's grid_sample composition.  valid [B, N] True = a real position."""
    B, N, d = h.shape
    L = len(spatial)
    hd = d // heads
    hq = r(h + pos)
    value = lin(sd, p + "value_proj", h, r)
    if defect != "no_value_mask":
        value = value.masked_fill(~valid[..., None], 0.0)
    value = value.view(B, N, heads, hd)
    off = lin(sd, p + "sampling_offsets", hq, r).view(B, N, heads, L, points, 2)
    aw = F.softmax(lin(sd, p + "attention_weights", hq, r).view(B, N, heads, L * points), -1).view(B, N, heads, L, points)
    sp = torch.tensor(spatial, dtype=torch.long, device=h.device)
    norm = torch.stack([sp[..., 0], sp[..., 1]], -1) if defect == "swap_normalizer" else torch.stack([sp[..., 1], sp[..., 0]], -1)
    loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    grids = 2 * loc - 1
    vals = value.split([hh * ww for hh, ww in spatial], dim=1)
    sampled = []
    for l, (hh, ww) in enumerate(spatial):
        vl = vals[l].flatten(2).transpose(1, 2).reshape(B * heads, hd, hh, ww)
        gl = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)
        sampled.append(F.grid_sample(vl, gl, mode="bilinear", padding_mode="zeros", align_corners=(defect == "align_corners")))
    aw = aw.transpose(1, 2).reshape(B * heads, 1, N, L * points)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * aw).sum(-1).view(B, heads * hd, N).transpose(1, 2).contiguous()
    return lin(sd, p + "output_proj", r(out), r)


def forward(sd, cfg, feature_maps, pixel_mask, text_hidden_states, text_token_mask, text_self_attention_masks, position_ids,
            twin=None, defect=None) -> dict:
    """-> dict(vision_states, text_states: the per-layer tuples (input of layer 0 first, the last state last), neck_maps, spatial, ...)."""
    r = (lambda x: x.to(twin).float()) if twin is not None else (lambda x: x)
    eps, heads = cfg["layer_norm_eps"], cfg["encoder_attention_heads"]
    if pixel_mask is None:
        pixel_mask = torch.ones((feature_maps[0].shape[0],) + tuple(cfg["image"]), dtype=torch.long, device=feature_maps[0].device)
    fms = [r(f.float()) for f in feature_maps]
    v, valid, pos, spatial, vr, maps = neck(sd, cfg, fms, pixel_mask, r)
    t = lin(sd, "text_projection", r(text_hidden_states.float()), r)
    ref = reference_points(spatial, vr, defect)
    tpos = r(text_position(position_ids, cfg["d_model"]).float())
    vs, ts = [v], [t]
    for i in range(cfg["encoder_layers"]):
        p = f"encoder.layers.{i}."
        f = p + "fusion_layer."
        # the library reassigns the variable: the residual is the LayerNorm-ed features, on both sides
        vn, tn = ln(sd, f + "layer_norm_vision", v, eps, r), ln(sd, f + "layer_norm_text", t, eps, r)
        dv, dt = bi_attention(sd, f + "attn.", vn, tn, ~valid, ~text_token_mask, heads // 2, r, defect)
        rv, rt = (v, t) if defect == "residual_unnormed" else (vn, tn)
        v = r(rv + r(sd[f + "vision_param"] * dv))
        t = r(rt + r(sd[f + "text_param"] * dt))
        t = text_enhancer(sd, p + "text_enhancer_layer.", t, text_self_attention_masks, tpos, heads // 2, cfg["encoder_ffn_dim"] // 2, eps, r, defect)
        m = p + "deformable_layer."
        v = ln(sd, m + "self_attn_layer_norm", r(v + msdeform(sd, m + "self_attn.", v, pos, valid, ref, spatial, heads, cfg["encoder_n_points"], r, defect)), eps, r)
        y = lin(sd, m + "fc2", r(F.relu(lin(sd, m + "fc1", v, r))), r)
        v = ln(sd, m + "final_layer_norm", r(v + y), eps, r)
        vs.append(v)
        ts.append(t)
    return dict(vision_states=tuple(vs), text_states=tuple(ts), neck_maps=maps, spatial=spatial, valid_ratios=vr, mask_flatten=valid,
                vision_position_embedding=pos, reference_points=ref)
