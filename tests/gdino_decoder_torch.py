"""GroundingDINO's query selection, decoder and heads (transformers' GroundingDinoModel.forward from "prepare decoder inputs" on,
GroundingDinoDecoder, the head loop of GroundingDinoForObjectDetection.forward) in plain fp32 torch, written literally: grid_sample,
masked_fill, the additive finfo.min mask of the text cross-attention.  The oracle of omg_amd/gdino_decoder.py
(tests/test_gdino_decoder.py pins it to a fixture made by the live library classes; tests/test_gdino_decoder_gpu.py holds the HIP
module to it).

`forward(sd, cfg, ...)` takes the library's state-dict keys without a prefix (the box heads under `decoder.bbox_embed.{i}`).
`twin=dtype` rounds every operation's result to the 16-bit type where the HIP module stores one (the weights are expected rounded by
the caller; scores, logits, references and boxes stay fp32 there and here).  `defect=` names one deliberate mistake
(tests/golden/make_golden_gdino_decoder.py proves that the fixture sees each of them).
"""
import math

import torch
import torch.nn.functional as F

from tests.gdino_torch import lin, ln, rel_rms  # noqa: F401

DEFECTS = ("box_head_normed_in_decoder", "box_head_unnormed_in_head", "same_level_reference", "no_logit_eps", "no_text_key_mask",
           "no_value_mask", "valid_ratio_one", "point_sampling", "swap_sine_xy", "pos_on_self_values", "residual_before_norm")

_BASE = dict(d_model=256, decoder_attention_heads=8, decoder_ffn_dim=2048, decoder_n_points=4, num_feature_levels=4, decoder_layers=2,
             activation_function="relu", layer_norm_eps=1e-5, max_text_len=256, query_dim=4, two_stage=True, embedding_init_target=True)

_SMALL = {
    # sample 1's pixel mask pads right and bottom: padded and invalid proposals exist; T = 11, two padded tokens in sample 0
    "a": dict(grids=[(13, 19), (7, 10), (4, 5), (2, 3)], B=2, T=11, padded=[2, 0], pixel_pad=True, num_queries=70, decoder_bbox_embed_share=False),
    "b": dict(grids=[(9, 25), (5, 13), (3, 7), (2, 4)], B=2, T=37, padded=[0, 0], pixel_pad=False, num_queries=19, decoder_bbox_embed_share=True),
    # b with 6 queries: the cut of the selection lies where the scores are sparse enough for a gap of 20 bf16 rounding errors
    "c": dict(grids=[(9, 25), (5, 13), (3, 7), (2, 4)], B=2, T=37, padded=[0, 0], pixel_pad=False, num_queries=6, decoder_bbox_embed_share=True),
}


def small_cfg(name: str) -> dict:
    c = dict(_BASE)
    c.update(_SMALL[name])
    c["name"] = name
    return c


def shapes(cfg: dict) -> dict:
    d, ffn, H8, L, P = cfg["d_model"], cfg["decoder_ffn_dim"], cfg["decoder_attention_heads"], cfg["num_feature_levels"], cfg["decoder_n_points"]
    out = {"query_position_embeddings.weight": (cfg["num_queries"], d)}

    def li(n, o, i):
        out[n + ".weight"], out[n + ".bias"] = (o, i), (o,)

    def norm(n):
        out[n + ".weight"], out[n + ".bias"] = (d,), (d,)

    def box(n):
        li(n + ".layers.0", d, d), li(n + ".layers.1", d, d), li(n + ".layers.2", 4, d)

    li("enc_output", d, d), norm("enc_output_norm"), box("encoder_output_bbox_embed")
    li("decoder.reference_points_head.layers.0", d, 2 * d), li("decoder.reference_points_head.layers.1", d, d), norm("decoder.layer_norm")
    for i in range(cfg["decoder_layers"]):
        p = f"decoder.layers.{i}."
        for a in ("self_attn", "encoder_attn_text"):
            for n in ("query", "key", "value", "out_proj"):
                li(p + f"{a}.{n}", d, d)
        li(p + "encoder_attn.sampling_offsets", H8 * L * P * 2, d), li(p + "encoder_attn.attention_weights", H8 * L * P, d)
        li(p + "encoder_attn.value_proj", d, d), li(p + "encoder_attn.output_proj", d, d)
        for n in ("self_attn_layer_norm", "encoder_attn_text_layer_norm", "encoder_attn_layer_norm", "final_layer_norm"):
            norm(p + n)
        li(p + "fc1", ffn, d), li(p + "fc2", d, ffn)
        box(f"decoder.bbox_embed.{i}")
    return out


def seed_state(cfg: dict, seed: int) -> dict:
    """Seeded weights under which nothing vanishes: Linear weights N(0, g^2 / fan_in) with gains that leave the softmaxes far from
    uniform and the offsets at a few eighths of a box, box deltas of order 1, norm weights around 1.  With decoder_bbox_embed_share
    every decoder.bbox_embed.{i} holds the tensors of index 0."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes(cfg).items():
        if "norm" in k and k.endswith(".weight"):
            v = 1.0 + 0.2 * torch.randn(s, generator=g)
        elif k.endswith(".bias"):
            v = (1.5 if "sampling_offsets" in k else 0.1) * torch.randn(s, generator=g)
        elif k == "query_position_embeddings.weight":
            v = torch.randn(s, generator=g)
        else:
            gain = 1.0
            if "sampling_offsets" in k or "attention_weights" in k or ".query" in k or ".key" in k:
                gain = 2.0
            v = torch.randn(s, generator=g) * gain / math.sqrt(s[-1])
        sd[k] = v
    if cfg["decoder_bbox_embed_share"]:
        for k in list(sd):
            if k.startswith("decoder.bbox_embed.") and not k.startswith("decoder.bbox_embed.0."):
                sd[k] = sd["decoder.bbox_embed.0." + k.split(".", 3)[3]].clone()
    return sd


def seeded_inputs(cfg: dict, seed: int) -> dict:
    """Encoder outputs on the grid of eighths (int8 / 8), the masks and the valid ratios of `cfg`."""
    g = torch.Generator().manual_seed(seed)
    B, T, grids = cfg["B"], cfg["T"], cfg["grids"]
    N = sum(h * w for h, w in grids)
    q8 = lambda t: torch.clamp(torch.round(t * 8.0), -127, 127) / 8.0
    memory = q8(torch.randn(B, N, cfg["d_model"], generator=g))
    text = q8(torch.randn(B, T, cfg["d_model"], generator=g))
    masks = []
    for h, w in grids:
        m = torch.ones(B, h, w, dtype=torch.bool)
        if cfg["pixel_pad"]:                 # sample 1: the last row and the last column of every level (59 rows, fewer than num_queries)
            m[1, h - 1:, :] = False
            m[1, :, w - 1:] = False
        masks.append(m)
    token_mask = torch.ones(B, T, dtype=torch.bool)
    for b, n in enumerate(cfg["padded"]):
        if n:
            token_mask[b, T - n:] = False
    vr = torch.stack([torch.stack([m[:, 0, :].sum(1).float() / m.shape[2], m[:, :, 0].sum(1).float() / m.shape[1]], -1) for m in masks], 1)
    return dict(memory=memory, text=text, mask_flatten=torch.cat([m.flatten(1) for m in masks], 1), text_token_mask=token_mask,
                spatial=[tuple(s) for s in grids], valid_ratios=vr)


# ------------------------------------------------------------------ the pieces
def proposals(mask_flatten, spatial):
    """generate_encoder_output_proposals without its Linear: (logits [B, N, 4] with +inf on padded / invalid rows, keep [B, N])."""
    B = mask_flatten.shape[0]
    padding = ~mask_flatten
    out, s = [], 0
    for level, (h, w) in enumerate(spatial):
        m = padding[:, s:s + h * w].view(B, h, w, 1)
        vh, vw = torch.sum(~m[:, :, 0, 0], 1), torch.sum(~m[:, 0, :, 0], 1)
        gy, gx = torch.meshgrid(torch.linspace(0, h - 1, h, dtype=torch.float32), torch.linspace(0, w - 1, w, dtype=torch.float32), indexing="ij")
        grid = torch.cat([gx.unsqueeze(-1), gy.unsqueeze(-1)], -1)
        scale = torch.cat([vw.unsqueeze(-1), vh.unsqueeze(-1)], 1).view(B, 1, 1, 2)
        grid = (grid.unsqueeze(0).expand(B, -1, -1, -1) + 0.5) / scale
        wh = torch.ones_like(grid) * 0.05 * (2.0 ** level)
        out.append(torch.cat((grid, wh), -1).view(B, -1, 4))
        s += h * w
    p = torch.cat(out, 1)
    valid = ((p > 0.01) & (p < 0.99)).all(-1, keepdim=True)
    p = torch.log(p / (1 - p))
    p = p.masked_fill(padding.unsqueeze(-1), float("inf")).masked_fill(~valid, float("inf"))
    return p, valid[..., 0] & mask_flatten


def sine_embed(pos, defect=None):
    """encode_sinusoidal_position_embedding(pos [.., 4], 128): blocks y, x, w, h."""
    dim_t = torch.arange(128, dtype=torch.float32)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / 128)
    es = [c[..., None] * (2 * math.pi) / dim_t for c in pos.unbind(-1)]
    es = [torch.stack((e[..., 0::2].sin(), e[..., 1::2].cos()), dim=-1).flatten(-2) for e in es]
    if defect != "swap_sine_xy":
        es[0], es[1] = es[1], es[0]
    return torch.cat(es, dim=-1)


def box_head(sd, name, x, r):
    """GroundingDinoMLPPredictionHead: the hidden Linears round as stored, the last one stays fp32 (it runs inside the reference step)."""
    h = r(F.relu(lin(sd, name + ".layers.1", r(F.relu(lin(sd, name + ".layers.0", x, r))), r)))
    return F.linear(h, sd[name + ".layers.2.weight"], sd[name + ".layers.2.bias"])


def logit(x, defect=None):
    return torch.special.logit(x, eps=None if defect == "no_logit_eps" else 1e-5)


def mha(sd, p, q_in, k_in, v_in, key_pad, heads, r):
    """GroundingDinoMultiheadAttention; key_pad [B, Nk] True = padded (the library adds finfo.min there)."""
    B, Nq, d = q_in.shape
    hd = d // heads
    sh = lambda x: x.view(B, -1, heads, hd).transpose(1, 2)
    q, k, v = sh(lin(sd, p + "query", q_in, r)), sh(lin(sd, p + "key", k_in, r)), sh(lin(sd, p + "value", v_in, r))
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    if key_pad is not None:
        s = s + key_pad[:, None, None, :].float() * torch.finfo(torch.float32).min
    a = r(F.softmax(s, dim=-1))
    o = r(torch.matmul(a, v)).permute(0, 2, 1, 3).reshape(B, Nq, d)
    return lin(sd, p + "out_proj", o, r)


def msdeform_box(sd, p, hq, memory, valid, ref_input, spatial, heads, points, r, defect=None):
    """GroundingDinoMultiscaleDeformableAttention with 4-coordinate reference points and the library's grid_sample composition."""
    B, Q, d = hq.shape
    N, L, hd = memory.shape[1], len(spatial), d // heads
    value = lin(sd, p + "value_proj", memory, r)
    if defect != "no_value_mask":
        value = value.masked_fill(~valid[..., None], 0.0)
    value = value.view(B, N, heads, hd)
    off = lin(sd, p + "sampling_offsets", hq, r).view(B, Q, heads, L, points, 2)
    aw = F.softmax(lin(sd, p + "attention_weights", hq, r).view(B, Q, heads, L * points), -1).view(B, Q, heads, L, points)
    if defect == "point_sampling":
        norm = torch.tensor([[w, h] for h, w in spatial], dtype=torch.float32)
        loc = ref_input[:, :, None, :, None, :2] + off / norm[None, None, None, :, None, :]
    else:
        loc = ref_input[:, :, None, :, None, :2] + off / points * ref_input[:, :, None, :, None, 2:] * 0.5
    grids = 2 * loc - 1
    vals = value.split([hh * ww for hh, ww in spatial], dim=1)
    sampled = []
    for l, (hh, ww) in enumerate(spatial):
        vl = vals[l].flatten(2).transpose(1, 2).reshape(B * heads, hd, hh, ww)
        gl = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)
        sampled.append(F.grid_sample(vl, gl, mode="bilinear", padding_mode="zeros", align_corners=False))
    aw = aw.transpose(1, 2).reshape(B * heads, 1, Q, L * points)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * aw).sum(-1).view(B, heads * hd, Q).transpose(1, 2).contiguous()
    return lin(sd, p + "output_proj", r(out), r)


def forward(sd, cfg, memory, text, mask_flatten, text_token_mask, spatial, valid_ratios, topk_proposals=None, twin=None, defect=None, scores_only=False) -> dict:
    """memory [B, N, 256] / text [B, T, 256]: the enhancer's last states; mask_flatten [B, N] True = a real position; text_token_mask
    [B, T] True = a real token.  -> dict(scores [B, N], topk_proposals, init_reference_points, states (per layer, normed), pre_norm_states,
    references (per layer), logits / pred_boxes (per level))."""
    r = (lambda x: x.to(twin).float()) if twin is not None else (lambda x: x)
    eps, heads, Q, NL = cfg["layer_norm_eps"], cfg["decoder_attention_heads"], cfg["num_queries"], cfg["decoder_layers"]
    B, N, d = memory.shape
    memory, text = r(memory.float()), r(text.float())
    vr = torch.ones_like(valid_ratios) if defect == "valid_ratio_one" else valid_ratios
    text_pad = None if defect == "no_text_key_mask" else ~text_token_mask

    prop, keep = proposals(mask_flatten, spatial)
    oq = ln(sd, "enc_output_norm", lin(sd, "enc_output", memory.masked_fill(~keep[..., None], 0.0), r), eps, r)
    s = oq @ text.transpose(-1, -2)
    scores = s.masked_fill(~text_token_mask[:, None, :], float("-inf")).max(-1)[0]
    if scores_only:
        return dict(scores=scores)
    if topk_proposals is None:
        topk_proposals = torch.topk(scores, Q, dim=1)[1]
    sel = torch.gather(oq, 1, topk_proposals[..., None].expand(-1, -1, d))
    ref = (box_head(sd, "encoder_output_bbox_embed", sel, r) + torch.gather(prop, 1, topk_proposals[..., None].expand(-1, -1, 4))).sigmoid()
    init_ref = ref

    def contrastive(x):
        out = (x @ text.transpose(-1, -2)).masked_fill(~text_token_mask[:, None, :], float("-inf"))
        full = torch.full((B, x.shape[1], cfg["max_text_len"]), float("-inf"))
        full[..., :out.shape[-1]] = out
        return full

    h = r(sd["query_position_embeddings.weight"])[None].repeat(B, 1, 1)
    states, pre, refs = [], [], []
    for i in range(NL):
        p = f"decoder.layers.{i}."
        ref_input = ref[:, :, None] * torch.cat([vr, vr], -1)[:, None]
        emb = r(sine_embed(ref_input[:, :, 0, :], defect))
        pos = lin(sd, "decoder.reference_points_head.layers.1", r(F.relu(lin(sd, "decoder.reference_points_head.layers.0", emb, r))), r)
        hq = r(h + pos)
        x = r(h + mha(sd, p + "self_attn.", hq, hq, hq if defect == "pos_on_self_values" else h, None, heads, r))
        h = ln(sd, p + "self_attn_layer_norm", x, eps, r)
        res = x if defect == "residual_before_norm" else h
        h = ln(sd, p + "encoder_attn_text_layer_norm", r(res + mha(sd, p + "encoder_attn_text.", r(h + pos), text, text, text_pad, heads, r)), eps, r)
        y = msdeform_box(sd, p + "encoder_attn.", r(h + pos), memory, mask_flatten, ref_input, spatial, heads, cfg["decoder_n_points"], r, defect)
        h = ln(sd, p + "encoder_attn_layer_norm", r(h + y), eps, r)
        h = ln(sd, p + "final_layer_norm", r(h + lin(sd, p + "fc2", r(F.relu(lin(sd, p + "fc1", h, r))), r)), eps, r)
        hn = ln(sd, "decoder.layer_norm", h, eps, r)
        ref = (box_head(sd, f"decoder.bbox_embed.{i}", hn if defect == "box_head_normed_in_decoder" else h, r) + logit(ref, defect)).sigmoid()
        states.append(hn), pre.append(h), refs.append(ref)

    logits, boxes = [], []
    for l in range(NL):
        prev = (init_ref if l == 0 else refs[l - 1]) if defect != "same_level_reference" else refs[l]
        x = pre[l] if defect == "box_head_unnormed_in_head" else states[l]
        boxes.append((box_head(sd, f"decoder.bbox_embed.{l}", x, r) + logit(prev, defect)).sigmoid())
        logits.append(contrastive(states[l]))
    return dict(scores=scores, topk_proposals=topk_proposals, init_reference_points=init_ref, states=tuple(states), pre_norm_states=tuple(pre),
                references=tuple(refs), logits=tuple(logits), pred_boxes=tuple(boxes))
