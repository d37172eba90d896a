"""transformers' BertModel(add_pooling_layer=False) for inference in plain fp32 torch, written literally: three embedding rows summed and
normed, per layer the q / k / v Linears, scores / 8 under the additive finfo.min block mask, softmax, the output Linear with the residual
taken BEFORE its LayerNorm, the erf GELU on the intermediate Linear.  The oracle of omg_amd/bert.py (tests/test_bert.py pins it to the
fixture of the live library class; tests/test_bert_gpu.py holds the HIP module to it).

`forward(sd, cfg, ...)` takes the library's state-dict keys without a prefix and returns the state after the embeddings and after every
layer.  `twin=dtype` rounds every operation's result to the 16-bit type (the weights are expected rounded by the caller): the yardstick
of what 16-bit storage costs on a given input.  `defect=` names one deliberate mistake (tests/golden/make_golden_bert.py proves that the
fixture sees each of them).

The inputs are those GroundingDINO gives its text backbone: attention_mask [B, T, T] True = attend and the per-phrase position_ids of
generate_masks_with_special_tokens_and_transfer_map (omg_amd.gdino_decoder.text_masks_from_input_ids restates it; `text_masks` below is a
third, token-by-token statement the fixture's generator compares both with).
"""
import math

import torch
import torch.nn.functional as F

DEFECTS = ("no_block_mask", "arange_positions", "no_token_type", "residual_after_norm", "no_score_scale", "heads_interleaved",
           "gelu_on_output")
SPECIAL = (101, 102, 1012, 1029)

_SMALL = {
    # the real Linear shapes of BERT-base: 768 x 768, 2304 x 768 fused, 3072 x 768, 768 x 3072
    "a": dict(hidden=768, heads=12, inter=3072, layers=2, vocab=1100, positions=128, types=2, eps=1e-12, lengths=(6, 23, 70)),
    # K = 328 is a multiple of 8 but not of 32
    "b": dict(hidden=192, heads=3, inter=328, layers=3, vocab=1100, positions=300, types=2, eps=1e-12, lengths=(6, 23, 70, 256)),
}


def small_cfg(name: str) -> dict:
    c = dict(_SMALL[name])
    c["name"] = name
    return c


def hf_config_dict(cfg: dict) -> dict:
    return dict(hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"], intermediate_size=cfg["inter"], num_hidden_layers=cfg["layers"],
                vocab_size=cfg["vocab"], max_position_embeddings=cfg["positions"], type_vocab_size=cfg["types"], layer_norm_eps=cfg["eps"],
                hidden_act="gelu", position_embedding_type="absolute")


def rel_rms(x: torch.Tensor, ref: torch.Tensor) -> float:
    return math.sqrt(float(((x.double() - ref.double()) ** 2).mean()) / max(float((ref.double() ** 2).mean()), 1e-60))


def shapes(cfg: dict) -> dict:
    d, f = cfg["hidden"], cfg["inter"]
    out = {"embeddings.word_embeddings.weight": (cfg["vocab"], d), "embeddings.position_embeddings.weight": (cfg["positions"], d),
           "embeddings.token_type_embeddings.weight": (cfg["types"], d), "embeddings.LayerNorm.weight": (d,), "embeddings.LayerNorm.bias": (d,)}
    for i in range(cfg["layers"]):
        p = f"encoder.layer.{i}."
        for n, (o, k) in {"attention.self.query": (d, d), "attention.self.key": (d, d), "attention.self.value": (d, d),
                          "attention.output.dense": (d, d), "intermediate.dense": (f, d), "output.dense": (d, f)}.items():
            out[p + n + ".weight"], out[p + n + ".bias"] = (o, k), (o,)
        for n in ("attention.output.LayerNorm", "output.LayerNorm"):
            out[p + n + ".weight"], out[p + n + ".bias"] = (d,), (d,)
    return out


def seed_state(cfg: dict, seed: int) -> dict:
    """Seeded weights under which nothing of the encoder vanishes: embedding rows of order 1 in all three tables (the position and the
    token-type row weigh as much as the word), q / k gains that leave every softmax far from uniform, intermediate pre-activations of
    order 1 (where the erf GELU is far from both of its asymptotes), norm weights around 1."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes(cfg).items():
        if "embeddings.weight" in k:
            v = torch.randn(s, generator=g)
        elif "LayerNorm.weight" in k:
            v = 1.0 + 0.2 * torch.randn(s, generator=g)
        elif k.endswith(".bias"):
            v = 0.1 * torch.randn(s, generator=g)
        else:
            gain = 2.0 if (".query." in k or ".key." in k) else 1.0
            v = torch.randn(s, generator=g) * gain / math.sqrt(s[1])
        sd[k] = v
    return sd


def seeded_ids(cfg: dict, T: int, seed: int) -> dict:
    """Three captions of different lengths (T, about 0.7 T, about 0.45 T; at least 5 and 4), right padded with [PAD] = 0 to T: [CLS], words
    in phrases of 1 to 4 closed by '.' (1012) or '?' (1029), [SEP].  token_type_ids: 1 on the second half of caption 1's tokens, so that
    both rows of the table are read."""
    g = torch.Generator().manual_seed(seed)
    lens = [T, max(5, int(round(0.7 * T))), max(4, int(round(0.45 * T)))]
    ids = torch.zeros(3, T, dtype=torch.long)
    for b, n in enumerate(lens):
        row, run = [101], 0
        while len(row) < n - 1:
            limit = 1 + int(torch.randint(0, 4, (1,), generator=g))
            if run >= limit and len(row) < n - 2:
                row.append(1012 if int(torch.randint(0, 2, (1,), generator=g)) else 1029)
                run = 0
            else:
                w = 103 + int(torch.randint(0, 900, (1,), generator=g))
                row.append(w)
                run += 1
        if n >= 4 and row[-1] not in SPECIAL and len(row) >= 3:
            row[-1] = 1012                                  # the last phrase is closed before [SEP]
        row.append(102)
        ids[b, :n] = torch.tensor(row[:n])
    types = torch.zeros_like(ids)
    types[1, lens[1] // 2:lens[1]] = 1
    mask, pos = text_masks(ids)
    return dict(input_ids=ids, token_type_ids=types, attention_mask=mask, position_ids=pos, lengths=lens)


def text_masks(input_ids: torch.Tensor):
    """generate_masks_with_special_tokens_and_transfer_map of the library, token by token: [B, T, T] bool and [B, T] int64.  A token's
    block is named by the next special token at or behind it; a block closed at position 0 or T - 1, or not closed at all, is no block
    (its tokens see themselves only and sit at position 0); the position counts from the special token in front."""
    B, T = input_ids.shape
    mask = torch.eye(T, dtype=torch.bool)[None].repeat(B, 1, 1)
    pos = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        special = [int(x) in SPECIAL for x in input_ids[b]]
        nxt = [next((j for j in range(t, T) if special[j]), T) for t in range(T)]
        prev = [next((j for j in range(t, -1, -1) if special[j]), -1) for t in range(T)]
        valid = [n not in (0, T - 1, T) for n in nxt]
        for i in range(T):
            if valid[i]:
                pos[b, i] = max(i - prev[i] - 1, 0)
            for j in range(T):
                if nxt[i] == nxt[j] and valid[j]:
                    mask[b, i, j] = True
    return mask, pos


# ------------------------------------------------------------------ the pieces
def ln(sd, name, x, eps, r):
    return r(F.layer_norm(x, x.shape[-1:], sd[name + ".weight"], sd[name + ".bias"], eps))


def lin(sd, name, x, r):
    return r(F.linear(x, sd[name + ".weight"], sd[name + ".bias"]))


def embeddings(sd, cfg, input_ids, token_type_ids, position_ids, r, defect=None):
    e = "embeddings."
    if defect == "arange_positions":
        position_ids = torch.arange(input_ids.shape[1])[None].expand_as(input_ids)
    x = sd[e + "word_embeddings.weight"][input_ids]
    if defect != "no_token_type":
        x = r(x + sd[e + "token_type_embeddings.weight"][token_type_ids])
    x = r(x + sd[e + "position_embeddings.weight"][position_ids])
    return ln(sd, e + "LayerNorm", x, cfg["eps"], r)


def layer(sd, cfg, p, h, attention_mask, r, defect=None):
    B, T, d = h.shape
    H = cfg["heads"]
    D = d // H

    def split(x):
        if defect == "heads_interleaved":
            return x.view(B, T, D, H).permute(0, 3, 1, 2)
        return x.view(B, T, H, D).transpose(1, 2)

    q, k, v = (split(lin(sd, p + "attention.self." + n, h, r)) for n in ("query", "key", "value"))
    s = r(q @ k.transpose(-1, -2))
    if defect != "no_score_scale":
        s = r(s / math.sqrt(D))
    if defect != "no_block_mask":
        s = s + (~attention_mask[:, None]).float() * torch.finfo(torch.float32).min
    pr = r(torch.softmax(s, dim=-1))
    o = r(pr @ v)
    o = o.permute(0, 2, 3, 1).reshape(B, T, d) if defect == "heads_interleaved" else o.transpose(1, 2).reshape(B, T, d)
    a = lin(sd, p + "attention.output.dense", o, r)
    if defect == "residual_after_norm":
        h = r(ln(sd, p + "attention.output.LayerNorm", a, cfg["eps"], r) + h)
    else:
        h = ln(sd, p + "attention.output.LayerNorm", r(a + h), cfg["eps"], r)
    f = lin(sd, p + "intermediate.dense", h, r)
    if defect != "gelu_on_output":
        f = r(F.gelu(f))
    a = lin(sd, p + "output.dense", f, r)
    if defect == "gelu_on_output":
        a = r(F.gelu(a))
    if defect == "residual_after_norm":
        return r(ln(sd, p + "output.LayerNorm", a, cfg["eps"], r) + h)
    return ln(sd, p + "output.LayerNorm", r(a + h), cfg["eps"], r)


def forward(sd, cfg, input_ids, attention_mask, token_type_ids, position_ids, twin=None, defect=None) -> list:
    """-> [the embeddings' output, the state after layer 0, ...], each [B, T, hidden] fp32."""
    assert defect is None or defect in DEFECTS, defect
    r = (lambda x: x.to(twin).float()) if twin is not None else (lambda x: x)
    h = embeddings(sd, cfg, input_ids, token_type_ids, position_ids, r, defect)
    states = [h]
    for i in range(cfg["layers"]):
        h = layer(sd, cfg, f"encoder.layer.{i}.", h, attention_mask, r, defect)
        states.append(h)
    return states
