"""Checkpoint and LoRA file loaders — the on-disk formats on the caller's side of the hot path.

The reference gets its weights through diffusers: ``from_pretrained(..., variant="fp16")`` for the UNet / ControlNet
(/root/reference inference_lora.py:151-157) and ``pipe.load_lora_weights(path, weight_name="pytorch_lora_weights.safetensors",
adapter_name=...)`` per concept and for the optional style LoRA (inference_lora.py:160-169), which accepts three key
styles for the UNet part of a LoRA file:

* PEFT:        ``unet.<module path>.lora_A.weight`` / ``.lora_B.weight``           (diffusers >= 0.26 / peft saves)
* diffusers:   ``unet.<module path>.lora.down.weight`` / ``.lora.up.weight``        (and the attention-processor form
               ``unet.<attn path>.processor.<to_q|to_k|to_v|to_out>_lora.down.weight`` of diffusers <= 0.21)
* kohya-ss:    ``lora_unet_<module path with '.' -> '_'>.lora_down.weight`` / ``.lora_up.weight`` / ``.alpha``, where the
               module path is either diffusers' (``down_blocks_1_attentions_0_...``) or — what kohya-ss's SDXL trainer writes
               and what the concept files the reference ships with use (``chris-evans.safetensors`` etc., inference_lora.py
               ``--lora_path``) — the SGM/ldm block naming ``input_blocks_4_1_...`` / ``middle_block_1_...`` /
               ``output_blocks_3_1_...``, remapped here as diffusers' ``_maybe_map_sgm_blocks_to_diffusers`` does [recalled].

Convolution entries (kohya ``conv_dim``, LyCORIS "LoCon", PEFT ``target_modules`` naming ``conv1`` / ``conv2`` ...) come in the same
three key styles with a 4-D down weight ``[r, Cin, k, k]`` and an up weight ``[Cout, r, 1, 1]``; ``load_lora_adapter`` accepts them
for the convolutions of :func:`conv_module_paths`.

LyCORIS LoHa (``hada_w1_a [out, r]``, ``hada_w1_b [r, in k k]``, ``hada_w2_a``, ``hada_w2_b``; delta = (w1_a . w1_b) * (w2_a . w2_b)) and LoKr
(``lokr_w1 [a, b]`` or ``lokr_w1_a`` . ``lokr_w1_b``; ``lokr_w2 [c, d(, k, k)]`` or ``lokr_w2_a`` . ``lokr_w2_b``; delta = kron(w1, w2)) are
recognised in the kohya / LyCORIS namespace (diffusers and SGM module names), on the same Linear and convolution targets and on the text
encoders; a DoRA magnitude (``dora_scale [out, 1]`` / ``[out, 1, 1, 1]`` / ``[out]``, or PEFT's ``lora_magnitude_vector [out]`` with an optional
``.weight`` / adapter-name segment) on any of them or on a plain pair.  Such modules become :class:`omg_amd.lora.LoraTerm` entries of
``adapter.terms`` with the factor ``alpha / r`` (1 without ``alpha``; 1 for a LoKr of two full matrices whatever ``alpha`` holds) kept beside
the fp32 factors; a file of plain pairs only gives the adapter it always gave.  Refused by name, every message carrying the words
``LoHa / LoKr / Tucker``: Tucker forms (``lora_mid``, ``hada_t1``, ``hada_t2``, ``lokr_t2``), a ``dora_scale`` of shape ``[1, in]`` (LyCORIS's
over-input form, which PEFT does not have), two algebras on one module, an incomplete or mis-shaped factor set, a magnitude on a
text-encoder module.  The LoHa / LoKr rules follow LyCORIS's published behaviour and the DoRA rule PEFT's; neither package is pinned here.

All are mapped onto the module paths of :class:`omg_amd.unet.UNet2DConditionModel` (whose state-dict keys equal
diffusers', boundary B4) and returned as a :class:`omg_amd.lora.LoraAdapter`.  A per-layer ``alpha`` (kohya) is folded
into the up matrix (``B <- B * alpha / r``); per-layer ranks may differ (PEFT ``rank_pattern``).  Text-encoder entries
(``text_encoder.*`` / ``text_encoder_2.*``, ``lora_te1_*`` / ``lora_te2_*``) are parsed into ``adapter.text_encoder[1|2]``
(module paths of transformers' CLIP text models) — the reference encodes every region prompt with the concept LoRA active
on both text encoders (lora_pipeline.py:336-347); :func:`omg_amd.text_encoder.make_encode_prompt` applies them.

Nothing here touches the GPU: tensors stay on the host until ``LoraBank.build`` / ``load_state_dict`` moves them.
"""
from __future__ import annotations

import os
import re
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from .lora import LoraAdapter, LoraTerm
from .modules import Linear, lora_conv_targets


class LoaderError(ValueError):
    pass


def _read_tensors(path_or_dict) -> Dict[str, torch.Tensor]:
    if isinstance(path_or_dict, dict):
        return path_or_dict
    path = os.fspath(path_or_dict)
    if os.path.isdir(path):          # diffusers passes a directory + weight_name (inference_lora.py:161,167)
        path = os.path.join(path, "pytorch_lora_weights.safetensors")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    obj = torch.load(path, map_location="cpu", weights_only=True)
    return obj.get("state_dict", obj) if isinstance(obj, dict) else obj


# ---------------------------------------------------------------------------------------------- model checkpoints
def load_model_weights(model: torch.nn.Module, path_or_dict, *, strict: bool = True, prefix: str = "",
                       allow_extra: bool = False) -> List[str]:
    """Load a diffusers-layout checkpoint (``diffusion_pytorch_model[.fp16].safetensors`` of a UNet / ControlNet) into
    ``model``.  ``prefix`` strips a leading namespace (``"unet."`` for a whole-pipeline single file).  ``allow_extra``
    accepts a file that holds more than the model (a full VAE file for the decoder-only module) while still requiring every
    tensor of the model.  Shapes are checked before anything is copied; dtype follows the model (fp32 files are rounded
    once).  Returns the ignored keys."""
    sd = _read_tensors(path_or_dict)
    if prefix:
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    own = model.state_dict()
    missing = [k for k in own if k not in sd]
    extra = [k for k in sd if k not in own]
    if strict and (missing or (extra and not allow_extra)):
        raise LoaderError(f"checkpoint does not match {type(model).__name__}: {len(missing)} missing (e.g. {missing[:3]}), "
                          f"{len(extra)} unexpected (e.g. {extra[:3]})")
    bad = [(k, tuple(sd[k].shape), tuple(own[k].shape)) for k in own if k in sd and sd[k].shape != own[k].shape]
    if bad:
        raise LoaderError(f"shape mismatch for {len(bad)} tensors, first: {bad[0]}")
    model.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=strict)
    return extra


# ---------------------------------------------------------------------------------------------- LoRA files
_PEFT = re.compile(r"^(?:unet\.)?(?P<mod>.+)\.lora_(?P<ab>[AB])(?:\.[^.]+)?\.weight$")          # optional adapter name segment
_DIFF = re.compile(r"^(?:unet\.)?(?P<mod>.+)\.lora\.(?P<ab>down|up)\.weight$")
_PROC = re.compile(r"^(?:unet\.)?(?P<attn>.+)\.processor\.(?P<proj>to_q|to_k|to_v|to_out)_lora\.(?P<ab>down|up)\.weight$")
_KOHYA = re.compile(r"^lora_unet_(?P<flat>.+)\.(?P<what>lora_down\.weight|lora_up\.weight|alpha)$")
_KOHYA_TE = re.compile(r"^lora_te(?P<n>[12]?)_(?P<flat>.+)\.(?P<what>lora_down\.weight|lora_up\.weight|alpha)$")
_TE_MOD = re.compile(r"^text_encoder(?P<n>_2)?\.(?P<rest>.+)$")
_SGM = re.compile(r"^(?P<blk>input_blocks|output_blocks)_(?P<i>\d+)_(?P<j>\d+)_(?P<rest>.+)$")
_SGM_MID = re.compile(r"^middle_block_(?P<j>\d+)_(?P<rest>.+)$")
_SGM_RES = (("in_layers_0", "norm1"), ("in_layers_2", "conv1"), ("emb_layers_1", "time_emb_proj"), ("out_layers_0", "norm2"),
            ("out_layers_3", "conv2"), ("skip_connection", "conv_shortcut"))


def sgm_flat_to_diffusers_flat(flat: str, layers_per_block: int = 2) -> str:
    """``input_blocks_4_1_transformer_blocks_0_attn1_to_q`` -> ``down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q``.

    SGM numbering of the SDXL UNet: ``input_blocks.0`` is conv_in; input block ``i >= 1`` is layer ``(i-1) % (lpb+1)`` of down
    block ``(i-1) // (lpb+1)`` (the last layer of a group is the downsampler ``.0.op``); ``middle_block.{0,1,2}`` = resnet,
    transformer, resnet; output block ``i`` is layer ``i % (lpb+1)`` of up block ``i // (lpb+1)``.  Inside a block ``.0`` is the
    resnet and ``.1`` the transformer (``.1`` / ``.2`` of an output block without / with attention is the upsampler ``conv``).
    Names that are not SGM are returned unchanged."""
    n = layers_per_block + 1

    def resnet(rest):
        for a, b in _SGM_RES:
            if rest == a or rest.startswith(a + "_"):
                return b + rest[len(a):]
        return rest

    m = _SGM_MID.match(flat)
    if m:
        j, rest = int(m["j"]), m["rest"]
        if j == 1:
            return f"mid_block_attentions_0_{rest}"
        return f"mid_block_resnets_{j // 2}_{resnet(rest)}"
    m = _SGM.match(flat)
    if not m:
        return flat
    i, j, rest = int(m["i"]), int(m["j"]), m["rest"]
    if m["blk"] == "input_blocks":
        if i == 0:
            return flat
        b, l = (i - 1) // n, (i - 1) % n
        if rest.startswith("op_") or rest == "op":
            return f"down_blocks_{b}_downsamplers_0_conv" + rest[2:]
        return f"down_blocks_{b}_attentions_{l}_{rest}" if j == 1 else f"down_blocks_{b}_resnets_{l}_{resnet(rest)}"
    b, l = i // n, i % n
    if rest.startswith("conv_") or rest == "conv":
        return f"up_blocks_{b}_upsamplers_0_conv" + rest[4:]
    return f"up_blocks_{b}_attentions_{l}_{rest}" if j == 1 else f"up_blocks_{b}_resnets_{l}_{resnet(rest)}"


def linear_module_paths(unet: torch.nn.Module) -> List[str]:
    return [n for n, m in unet.named_modules() if isinstance(m, Linear)]


_CONV_BOUNDARY = ("conv_in", "conv_out")
_CONV_BOUNDARY_FLAT = ("conv_in", "conv_out", "input_blocks_0_0", "out_2")          # the same two layers in kohya's flat / SGM names
# other adapter algebras that share the lora_unet_* / PEFT namespaces (LyCORIS LoHa, LoKr, Tucker-decomposed LoCon, DoRA)
_FOREIGN = ("hada_", "lokr_", "lora_mid", "dora_scale", "lora_magnitude_vector")
_LYCO_WHAT = r"(?P<what>hada_w[12]_[ab]|hada_t[12]|lokr_w[12](?:_[ab])?|lokr_t2|lora_mid(?:\.weight)?|dora_scale)"
_LYCO = re.compile(r"^lora_unet_(?P<flat>.+)\." + _LYCO_WHAT + "$")
_LYCO_TE = re.compile(r"^lora_te(?P<n>[12]?)_(?P<flat>.+)\." + _LYCO_WHAT + "$")
_PEFT_MAG = re.compile(r"^(?P<mod>.+)\.lora_magnitude_vector(?:\.[^.]+){0,2}$")        # bare, .weight, .<adapter>, .<adapter>.weight
_TUCKER = ("lora_mid", "lora_mid.weight", "hada_t1", "hada_t2", "lokr_t2")
_HADA = ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")


def _family_error(key: str, reason: str) -> "LoaderError":
    return LoaderError(f"LoHa / LoKr / Tucker (lora_mid) / DoRA entry {key!r}: {reason}")


def _magnitude(key: str, t: torch.Tensor, n_out: Optional[int]) -> torch.Tensor:
    """DoRA's per-output-channel magnitude as fp32 ``[out]``: ``[out, 1]``, ``[out, 1, 1, 1]`` or ``[out]`` in the file.  LyCORIS's
    over-input form ``[1, in]`` has no PEFT counterpart and is refused by name."""
    shape = tuple(t.shape)
    if len(shape) == 2 and shape[0] == 1 and shape[1] > 1:
        raise _family_error(key, f"a magnitude of shape {shape} runs over the input axis (LyCORIS wd_on_out=False); only per-output-channel "
                                 f"magnitudes are supported")
    if not (len(shape) in (1, 2, 4) and all(d == 1 for d in shape[1:])) or (n_out is not None and shape[0] != n_out):
        raise _family_error(key, f"a magnitude of shape {shape} is not [out, 1], [out, 1, 1, 1] or [out]"
                                 + (f" with out = {n_out}" if n_out is not None else ""))
    return t.float().reshape(-1)


def _make_term(key: str, f: Dict[str, torch.Tensor], alpha: Optional[float], conv: Optional[Tuple[int, int, int]]) -> LoraTerm:
    """The LoHa / LoKr term of one module from its file entries ``f`` (suffix -> tensor, the magnitude excluded); ``conv`` =
    ``(Cin, Cout, k)`` of a convolution target, ``None`` for a Linear, whose own shape is checked when the bank is built."""
    names = set(f)
    hada, kron = sorted(n for n in names if n.startswith("hada_")), sorted(n for n in names if n.startswith("lokr_"))
    if hada and kron:
        raise _family_error(key, "LoHa and LoKr factors on one module; one algebra per module and file")
    taps = conv[2] * conv[2] if conv else 1
    if hada:
        if tuple(hada) != _HADA:
            raise _family_error(key, f"incomplete LoHa factor set: has {hada}, needs {list(_HADA)}")
        a1, b1, a2, b2 = (f[n] for n in _HADA)
        ok = all(t.dim() == 2 for t in (a1, b1, a2, b2)) and a1.shape[1] == b1.shape[0] and a2.shape[1] == b2.shape[0] \
            and a1.shape[0] == a2.shape[0] and b1.shape[1] == b2.shape[1] and min(a1.shape[1], a2.shape[1]) >= 1
        if ok and conv:
            ok = a1.shape[0] == conv[1] and b1.shape[1] == conv[0] * taps
        if not ok:
            raise _family_error(key, "LoHa factor shapes " + ", ".join(f"{n} {tuple(f[n].shape)}" for n in _HADA) + " are not [out, r], [r, in k k] twice"
                                     + (f" for a {conv[2]}x{conv[2]} convolution {conv[0]} -> {conv[1]}" if conv else ""))
        return LoraTerm("hada", {n: f[n] for n in _HADA}, alpha)
    ops_ = {}
    for w in ("lokr_w1", "lokr_w2"):
        full, fa, fb = w in names, w + "_a" in names, w + "_b" in names
        if full == (fa or fb) or fa != fb:
            raise _family_error(key, f"incomplete LoKr factor set: {w} needs either {w} or both {w}_a and {w}_b, has {kron}")
        ops_[w] = (f[w],) if full else (f[w + "_a"], f[w + "_b"])
    def shape_of(op):                                    # (rows, columns) of the operand, a 4-D w2 flattened to [c, d k k]
        if len(op) == 1:
            return op[0].shape[0], op[0][0].numel()
        return op[0].shape[0], op[1].shape[1]
    ok = all(t.dim() == 2 for op in ops_.values() for t in op if len(op) == 2) and ops_["lokr_w1"][0].dim() == 2 \
        and ops_["lokr_w2"][0].dim() in ((2, 4) if len(ops_["lokr_w2"]) == 1 else (2,)) \
        and all(op[0].shape[1] == op[1].shape[0] and op[0].shape[1] >= 1 for op in ops_.values() if len(op) == 2)
    if ok and conv:
        (a, b), (c, dk) = shape_of(ops_["lokr_w1"]), shape_of(ops_["lokr_w2"])
        w2 = ops_["lokr_w2"][0]
        ok = a * c == conv[1] and dk % taps == 0 and b * (dk // taps) == conv[0] and (len(ops_["lokr_w2"]) == 2 or taps == 1 or
                                                                                      (w2.dim() == 4 and tuple(w2.shape[2:]) == (conv[2], conv[2])))
    if not ok:
        raise _family_error(key, "LoKr factor shapes " + ", ".join(f"{n} {tuple(f[n].shape)}" for n in kron) + " do not give w1 [a, b] and w2 [c, d(, k, k)]"
                                 + (f" with a c = {conv[1]}, b d = {conv[0]}, k = {conv[2]}" if conv else ""))
    return LoraTerm("kron", {n: f[n] for n in kron}, alpha)


def conv_module_paths(unet: torch.nn.Module) -> Dict[str, Tuple[int, int, int]]:
    """``{module path: (Cin, Cout, k)}`` of the convolutions a LoRA may target: every 16-bit :class:`Conv2d` the slot kernel runs (resnet
    conv1 / conv2 / conv_shortcut, ``downsamplers.0.conv``, ``upsamplers.0.conv``).  ``conv_in`` / ``conv_out`` are not targets."""
    return {n: (m.cin, m.cout, m.ksize) for n, m in lora_conv_targets(unet).items()}


_TE_PROJ = ("q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2")


def _te_unflatten(flat: str) -> str:
    """``text_model_encoder_layers_0_self_attn_q_proj`` -> ``text_model.encoder.layers.0.self_attn.q_proj``."""
    m = re.match(r"^text_model_encoder_layers_(\d+)_(self_attn|mlp)_(\w+)$", flat)
    if not m or m[3] not in _TE_PROJ:
        raise LoaderError(f"unrecognised text-encoder LoRA module {flat!r}")
    return f"text_model.encoder.layers.{m[1]}.{m[2]}.{m[3]}"


def parse_lora_state_dict(sd: Dict[str, torch.Tensor], module_paths: Iterable[str], name: str = "lora",
                          layers_per_block: int = 2,
                          conv_paths: Optional[Dict[str, Tuple[int, int, int]]] = None) -> Tuple[LoraAdapter, List[str]]:
    """Key-style detection + mapping (see the module docstring).  Returns ``(adapter, skipped_keys)``; raises
    ``LoaderError`` for a UNet entry that names no Linear layer of ``module_paths`` and no convolution of ``conv_paths``
    (``{path: (Cin, Cout, k)}``, :func:`conv_module_paths`; ``None``: Linear targets only) or for a half-present pair.  With
    ``conv_paths`` it also raises, by name, for a down kernel that is not the base layer's, an up weight that is not 1x1 and an entry
    for ``conv_in`` / ``conv_out``.  LoHa / LoKr factors and DoRA magnitudes go to ``adapter.terms`` (module docstring); what is refused of
    them is refused by name.  ``skipped_keys`` lists what was neither UNet nor
    text-encoder material."""
    paths = set(module_paths)
    convs = dict(conv_paths or {})
    flat = {p.replace(".", "_"): p for p in list(paths) + list(convs)}
    # key = ("unet", module) or ("te", 1 | 2, module)
    down: Dict[tuple, torch.Tensor] = {}
    up: Dict[tuple, torch.Tensor] = {}
    alpha: Dict[tuple, float] = {}
    extra: Dict[tuple, Dict[str, torch.Tensor]] = {}       # LoHa / LoKr factors, Tucker cores and magnitudes per module, under their file suffix
    extra_key: Dict[tuple, str] = {}                       # the first such file key of a module, for messages
    skipped: List[str] = []

    def resolve(mod: str, key: str) -> str:
        if mod.endswith(".to_out") and mod + ".0" in paths:      # diffusers' Attention.to_out is [Linear, Dropout]
            mod = mod + ".0"
        if conv_paths is not None and mod in _CONV_BOUNDARY:
            raise LoaderError(f"LoRA entry {key!r} targets {mod!r}: conv_in / conv_out are not LoRA targets")
        if mod not in paths and mod not in convs:
            raise LoaderError(f"LoRA entry {key!r} targets {mod!r}, which is not a Linear layer of this UNet "
                              + ("(LoRA on conv layers is not supported)" if conv_paths is None else "nor one of its LoRA-capable convolutions"))
        return mod

    def put(mod: str, which: str, t: torch.Tensor, key: str):
        (down if which == "down" else up)[("unet", resolve(mod, key))] = t

    def kohya_module(flat_name: str, key: str) -> str:
        mod = flat.get(flat_name) or flat.get(sgm_flat_to_diffusers_flat(flat_name, layers_per_block))
        if mod is None and conv_paths is not None and flat_name in _CONV_BOUNDARY_FLAT:
            raise LoaderError(f"kohya LoRA entry {key!r} targets conv_in / conv_out, which are not LoRA targets")
        if mod is None:
            raise LoaderError(f"kohya LoRA entry {key!r} matches no Linear layer of this UNet "
                              f"(LoRA on conv layers is not supported)")
        return mod

    def put_extra(k: tuple, what: str, t: torch.Tensor, key: str):
        extra.setdefault(k, {})[what] = t
        extra_key.setdefault(k, key)

    def foreign(key: str, t: torch.Tensor):
        """A key of another algebra (LoHa, LoKr, Tucker) or a DoRA magnitude: kohya / LyCORIS names, or PEFT's magnitude vector."""
        m = _LYCO_TE.match(key)
        if m:
            put_extra(("te", 2 if m["n"] == "2" else 1, _te_unflatten(m["flat"])), m["what"], t, key)
            return
        m = _LYCO.match(key)
        if m:
            put_extra(("unet", kohya_module(m["flat"], key)), m["what"], t, key)
            return
        m = _PEFT_MAG.match(key)
        if m:
            if _TE_MOD.match(key):
                raise _family_error(key, "a DoRA magnitude on a text-encoder module is not supported")
            mod = m["mod"][5:] if m["mod"].startswith("unet.") else m["mod"]
            put_extra(("unet", resolve(mod, key)), "dora_scale", t, key)
            return
        raise _family_error(key, "not a key of the kohya / LyCORIS namespace (lora_unet_<module>.<factor>) nor PEFT's lora_magnitude_vector")

    def put_te(n: int, mod: str, which: str, t: torch.Tensor):
        (down if which == "down" else up)[("te", n, mod)] = t

    for key, t in sd.items():
        if any(f in key for f in _FOREIGN):
            foreign(key, t)
            continue
        m = _KOHYA_TE.match(key)
        if m:
            k = ("te", 2 if m["n"] == "2" else 1, _te_unflatten(m["flat"]))
            if m["what"] == "alpha":
                alpha[k] = float(t)
            else:
                put_te(k[1], k[2], "down" if m["what"].startswith("lora_down") else "up", t)
            continue
        m = _TE_MOD.match(key)
        if m:
            n, rest = (2 if m["n"] else 1), m["rest"]
            mm = (re.match(r"^(?P<mod>.+)\.lora_(?P<ab>[AB])(?:\.[^.]+)?\.weight$", rest)
                  or re.match(r"^(?P<mod>.+)\.(?:lora_linear_layer|lora)\.(?P<ab>down|up)\.weight$", rest))
            if mm:
                put_te(n, mm["mod"], {"A": "down", "B": "up"}.get(mm["ab"], mm["ab"]), t)
            else:
                skipped.append(key)
            continue
        m = _PROC.match(key)
        if m:
            put(f"{m['attn']}.{m['proj']}", m["ab"], t, key)
            continue
        m = _DIFF.match(key)
        if m:
            put(m["mod"], m["ab"], t, key)
            continue
        m = _PEFT.match(key)
        if m:
            put(m["mod"], "down" if m["ab"] == "A" else "up", t, key)
            continue
        m = _KOHYA.match(key)
        if m:
            mod = kohya_module(m["flat"], key)
            if m["what"] == "alpha":
                alpha[("unet", mod)] = float(t)
            else:
                put(mod, "down" if m["what"].startswith("lora_down") else "up", t, key)
            continue
        skipped.append(key)

    # ---- the other algebras and the magnitudes: one LoraTerm per module, refusals by name
    terms: Dict[str, LoraTerm] = {}
    te_terms: Dict[tuple, LoraTerm] = {}
    for k in sorted(extra, key=str):
        f, key = dict(extra[k]), extra_key[k]
        tucker = sorted(n for n in f if n in _TUCKER)
        if tucker:
            raise _family_error(key, f"Tucker-decomposed factors ({', '.join(tucker)}) are not supported")
        mag = f.pop("dora_scale", None)
        has_pair = k in down or k in up
        if f and has_pair:
            raise _family_error(key, "a plain lora_down / lora_up pair and LoHa / LoKr factors on one module; one algebra per module and file")
        if mag is not None and k[0] == "te":
            raise _family_error(key, "a DoRA magnitude on a text-encoder module is not supported")
        if not f and not has_pair:
            raise _family_error(key, "incomplete factor set: a magnitude without the factors of its delta")
        if not f:
            continue                                           # a magnitude on a plain pair: attached where the pairs are formed, below
        term = _make_term(key, f, alpha.get(k), convs.get(k[1]) if k[0] == "unet" else None)
        if mag is not None:
            term.magnitude = _magnitude(key, mag, term.out_features)
        if k[0] == "unet":
            terms[k[1]] = term
        else:
            te_terms[k] = term
    if not any(k[0] == "unet" for k in list(down) + list(up)) and not terms:
        raise LoaderError("no UNet LoRA entries found (expected PEFT lora_A/lora_B, diffusers lora.down/up or kohya lora_unet_* keys)")
    half = sorted(str(k) for k in set(down) ^ set(up))
    if half:
        raise LoaderError(f"LoRA pair incomplete for {half[:3]} ({len(half)} layers)")
    weights: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
    te: Dict[int, Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = {}
    for k in sorted(down, key=str):
        a, b = down[k].float(), up[k].float()
        if k[0] == "unet" and k[1] in convs:
            cin, cout, ks = convs[k[1]]
            if a.dim() != 4 or tuple(a.shape[1:]) != (cin, ks, ks):
                raise LoaderError(f"conv LoRA down weight of {k[1]}: {tuple(a.shape)} is not [r, {cin}, {ks}, {ks}] — the down kernel must be "
                                  f"the base layer's")
            if b.dim() == 4 and tuple(b.shape[2:]) != (1, 1):
                raise LoaderError(f"conv LoRA up weight of {k[1]}: {tuple(b.shape)} is not a 1x1 convolution")
            if b.dim() not in (2, 4) or tuple(b.shape[:2]) != (cout, a.shape[0]):
                raise LoaderError(f"LoRA shapes of {k}: down {tuple(a.shape)}, up {tuple(b.shape)}")
            b = b.reshape(cout, a.shape[0])
            if k in extra:                                       # a DoRA magnitude: the pair stays a term, alpha / r unfolded
                terms[k[1]] = LoraTerm("plain", {"lora_down": a, "lora_up": b}, alpha.get(k), _magnitude(extra_key[k], extra[k]["dora_scale"], cout))
                continue
            if k in alpha:
                b = b * (alpha[k] / a.shape[0])
            weights[k[1]] = (a, b)
            continue
        if a.dim() != 2 or b.dim() != 2 or b.shape[1] != a.shape[0]:
            raise LoaderError(f"LoRA shapes of {k}: down {tuple(a.shape)}, up {tuple(b.shape)}")
        if k in extra:
            terms[k[1]] = LoraTerm("plain", {"lora_down": a, "lora_up": b}, alpha.get(k), _magnitude(extra_key[k], extra[k]["dora_scale"], b.shape[0]))
            continue
        if k in alpha:
            b = b * (alpha[k] / a.shape[0])
        if k[0] == "unet":
            weights[k[1]] = (a, b)
        else:
            te.setdefault(k[1], {})[k[2]] = (a, b)
    for k, term in te_terms.items():
        te.setdefault(k[1], {})[k[2]] = term
    return LoraAdapter(name, weights, alpha=None, text_encoder=te, terms=terms), skipped


def load_lora_adapter(unet: torch.nn.Module, path_or_dict, adapter_name: Optional[str] = None) -> LoraAdapter:
    """``pipe.load_lora_weights(path, adapter_name=...)`` for the UNet half: returns the adapter, ready for
    ``LoraBank(unet, [adapters...]).build(...)``.  The default name follows the reference
    (``lora_path.split('/')[-1].split('.')[0]``, inference_lora.py:166)."""
    if adapter_name is None:
        if isinstance(path_or_dict, dict):
            adapter_name = "lora"
        else:
            adapter_name = os.fspath(path_or_dict).rstrip("/").split("/")[-1].split(".")[0]
    lpb = getattr(getattr(unet, "config", None), "layers_per_block", 2)
    adapter, skipped = parse_lora_state_dict(_read_tensors(path_or_dict), linear_module_paths(unet), adapter_name, lpb,
                                             conv_paths=conv_module_paths(unet))
    adapter.skipped_keys = skipped
    return adapter


# ---------------------------------------------------------------------------------------------- writers (tests, tooling)
def lora_state_dict(adapter: LoraAdapter, style: str = "peft") -> Dict[str, torch.Tensor]:
    """The inverse mapping, in any of the three key styles (used by the round-trip tests and to export synthetic adapters);
    the text-encoder half, when present, is written in the same style."""
    out: Dict[str, torch.Tensor] = {}
    for n, mods in adapter.text_encoder.items():
        pre = "text_encoder" if n == 1 else "text_encoder_2"
        for mod, pair in mods.items():
            if isinstance(pair, LoraTerm):
                _write_term(out, f"lora_te{n}_" + mod.replace(".", "_"), pair, style)
                continue
            a, b = pair[0].contiguous(), pair[1].contiguous()
            if style == "peft":
                out[f"{pre}.{mod}.lora_A.weight"], out[f"{pre}.{mod}.lora_B.weight"] = a, b
            elif style == "diffusers":
                out[f"{pre}.{mod}.lora_linear_layer.down.weight"], out[f"{pre}.{mod}.lora_linear_layer.up.weight"] = a, b
            else:
                flat = f"lora_te{n}_" + mod.replace(".", "_")
                out[f"{flat}.lora_down.weight"], out[f"{flat}.lora_up.weight"] = a, b
                out[f"{flat}.alpha"] = torch.tensor(float(a.shape[0]))
    for mod, (a, b) in adapter.weights.items():
        a, b = a.contiguous(), b.contiguous()
        if a.dim() == 4:                      # a convolution target: files hold the up weight as a 1x1 conv
            b = b.reshape(b.shape[0], b.shape[1], 1, 1)
        if style == "peft":
            out[f"unet.{mod}.lora_A.weight"], out[f"unet.{mod}.lora_B.weight"] = a, b
        elif style == "diffusers":
            out[f"unet.{mod}.lora.down.weight"], out[f"unet.{mod}.lora.up.weight"] = a, b
        elif style == "kohya":
            flat = "lora_unet_" + mod.replace(".", "_")
            out[f"{flat}.lora_down.weight"], out[f"{flat}.lora_up.weight"] = a, b
            out[f"{flat}.alpha"] = torch.tensor(float(adapter.alpha if adapter._alpha_given else a.shape[0]))
        else:
            raise ValueError(style)
    for mod, term in adapter.terms.items():
        _write_term(out, "lora_unet_" + mod.replace(".", "_"), term, style)
    return out


def _write_term(out: Dict[str, torch.Tensor], flat: str, term: LoraTerm, style: str) -> None:
    """A LoHa / LoKr / DoRA term under its kohya / LyCORIS keys — the only namespace that has names for all of them."""
    if style != "kohya":
        raise ValueError(f"{flat}: LoHa / LoKr / DoRA terms are written in the kohya style only, not {style!r}")
    for n, t in term.factors.items():
        t = t.contiguous()
        if n == "lora_up" and term.factors["lora_down"].dim() == 4:
            t = t.reshape(t.shape[0], t.shape[1], 1, 1)
        out[f"{flat}.{n}" + (".weight" if n in ("lora_down", "lora_up") else "")] = t
    if term.alpha is not None:
        out[f"{flat}.alpha"] = torch.tensor(term.alpha)
    if term.magnitude is not None:
        conv = any(t.dim() == 4 for t in term.factors.values())
        out[f"{flat}.dora_scale"] = term.magnitude.reshape(-1, 1, 1, 1) if conv else term.magnitude.reshape(-1, 1)
