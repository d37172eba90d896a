"""The Swin backbone on the HIP kernels: ``transformers.SwinBackbone`` for inference — the image backbone of GroundingDINO
(``GroundingDINO_SwinB.cfg.py``: Swin-B, window 12), in front of the detector's text encoder, feature enhancer and decoder.

Parameters are kept under the installed library's own key names (``swin.embeddings.*``, ``swin.encoder.layers.L.blocks.B.attention.
{q_proj,k_proj,v_proj,o_proj}``, ``...relative_position_bias.relative_position_bias_table``, ``mlp.fc1 / fc2``, ``downsample.{norm,
reduction}``, ``hidden_states_norms.stageN``); ``load_state_dict`` also takes the names Hub checkpoints carry (``attention.self.query``,
``attention.output.dense``, ``intermediate.dense``, ``output.dense``) and a prefix, and :func:`swin_from_groundingdino` maps the
original package's ``backbone.0.*`` keys.  NCHW pixel values in (fp32 or the storage dtype, any size), image-order rows
``[B * h * w, C]`` inside, NCHW feature maps out.

  patch embedding (4 x 4, stride 4)      -> omg_swin_patch_embed (the patch rows, implicit zero padding, K 48 padded to 64) + omg_gemm
  LayerNorms                             -> omg_layernorm
  q / k / v (ONE [3C, C] weight), o_proj, fc1, fc2 -> omg_gemm: bias and the shortcut in its epilogue
  (shifted-)window attention             -> omg_attn_swin on the fused QKV rows: no roll, pad, partition or reverse pass, no bias, mask
                                            or score tensor (a padded position is a key with k | v = the k | v slices of the QKV
                                            bias, which is what zero padding AFTER layernorm_before makes of it)
  GELU of the MLP                        -> omg_gelu_erf, in place
  patch merging                          -> omg_swin_merge_ln (gather + LayerNorm) + omg_gemm (4C -> 2C, no bias)

The window is never clamped to the grid: ``SwinBackbone`` runs its encoder with ``always_partition=True``; ``SwinModel`` (which clamps)
is not built.  Inference only.  There is no CPU path: ``forward`` on a CPU tensor raises.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from . import ops
from ._checkpoint import FlatWeights

__all__ = ["SwinBackbone", "SwinBackboneOutput", "swin_from_groundingdino", "check_config"]

HEAD_DIM = 32
PATCH_K = 64            # 3 * 4 * 4 = 48 columns, padded so that a patch row is a whole number of 64-byte lines

_HUB_NAMES = ((".attention.self.query.", ".attention.q_proj."), (".attention.self.key.", ".attention.k_proj."),
              (".attention.self.value.", ".attention.v_proj."), (".attention.output.dense.", ".attention.o_proj."),
              (".attention.self.relative_position_bias_table", ".attention.relative_position_bias.relative_position_bias_table"),
              (".intermediate.dense.", ".mlp.fc1."), (".output.dense.", ".mlp.fc2."))


def _refuse(key: str, why: str):
    raise L.OmgHipError(f"SwinBackbone: config key '{key}': {why}")


def check_config(config) -> dict:
    """``SwinConfig`` / its dict / a ``GroundingDinoConfig`` (its ``backbone_config``) -> the plain dict the module keeps.  Anything the
    kernels do not compute is refused with the key named."""
    if hasattr(config, "backbone_config") and getattr(config, "backbone_config") is not None:
        config = config.backbone_config
    cfg = dict(config.to_dict() if hasattr(config, "to_dict") else config)
    if isinstance(cfg.get("backbone_config"), dict):
        cfg = dict(cfg["backbone_config"])
    if cfg.get("model_type", "swin") != "swin":
        _refuse("model_type", f"'{cfg['model_type']}' is not a Swin backbone")
    if cfg.get("use_absolute_embeddings", False):
        _refuse("use_absolute_embeddings", "absolute position embeddings are not built")
    if not cfg.get("qkv_bias", True):
        _refuse("qkv_bias", "projections without a bias are not built (the padded keys are the bias slices)")
    if cfg.get("hidden_act", "gelu") != "gelu":
        _refuse("hidden_act", f"'{cfg['hidden_act']}' has no kernel (omg_gelu_erf is the erf GELU)")
    ps = cfg.get("patch_size", 4)
    if ps != 4 and tuple(ps if isinstance(ps, (list, tuple)) else (ps,)) != (4, 4):
        _refuse("patch_size", f"{ps} has no kernel (omg_swin_patch_embed cuts 4 x 4 patches)")
    if cfg.get("num_channels", 3) != 3:
        _refuse("num_channels", f"{cfg['num_channels']} has no kernel (omg_swin_patch_embed reads 3 channels)")
    E, depths, heads = int(cfg.get("embed_dim", 96)), list(cfg.get("depths", [2, 2, 6, 2])), list(cfg.get("num_heads", [3, 6, 12, 24]))
    if len(depths) != len(heads):
        _refuse("num_heads", f"{len(heads)} entries beside {len(depths)} depths")
    for li, nh in enumerate(heads):
        if nh < 1 or (E << li) != nh * HEAD_DIM:
            _refuse("num_heads", f"stage {li + 1}: width {E << li} over {nh} heads is head_dim {(E << li) / max(nh, 1):g}; omg_attn_swin is built "
                                 f"for head_dim {HEAD_DIM} ('embed_dim' {E})")
    S = cfg.get("window_size", 7)
    if S not in (7, 12):
        _refuse("window_size", f"{S} has no kernel (omg_attn_swin is built for 7 and 12)")
    ratio = float(cfg.get("mlp_ratio", 4.0))
    for li in range(len(depths)):
        if int(ratio * (E << li)) % 8 or int(ratio * (E << li)) < 8:
            _refuse("mlp_ratio", f"{ratio:g} makes the MLP of stage {li + 1} {int(ratio * (E << li))} wide; omg_gemm takes multiples of 8")
    for k in ("hidden_dropout_prob", "attention_probs_dropout_prob", "drop_path_rate"):
        cfg.setdefault(k, 0.0)          # inference: identity, whatever the value; train() is refused
    names = ["stem"] + [f"stage{i + 1}" for i in range(len(depths))]
    of, oi = cfg.get("out_features"), cfg.get("out_indices")
    if of is None:
        of = [names[i] for i in oi] if oi is not None else [names[-1]]
    of = list(of)
    for st in of:
        if st not in names[1:]:
            _refuse("out_features", f"'{st}' is not one of {names[1:]} (the stem as a feature map is not built)")
    return dict(embed_dim=E, depths=depths, num_heads=heads, window_size=int(S), mlp_ratio=ratio, layer_norm_eps=float(cfg.get("layer_norm_eps", 1e-5)),
                out_features=of, stage_names=names)


def swin_from_groundingdino(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The Swin part of the original GroundingDINO package's checkpoint (``groundingdino_swinb_cogcoor.pth``: ``backbone.0.*``, a leading
    ``module.`` stripped) under this module's names; ``attn.qkv`` is split in q, k, v order.  Keys outside ``backbone.0.`` are dropped."""
    if "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    out: Dict[str, torch.Tensor] = {}
    leaf_map = {"norm1": "layernorm_before", "norm2": "layernorm_after", "attn.proj": "attention.o_proj", "mlp.fc1": "mlp.fc1", "mlp.fc2": "mlp.fc2"}
    for k, v in sd.items():
        if k.startswith("module."):
            k = k[len("module."):]
        if not k.startswith("backbone.0."):
            continue
        k = k[len("backbone.0."):]
        p = k.split(".")
        if p[0] == "patch_embed":
            out["swin.embeddings." + ("patch_embeddings.projection." if p[1] == "proj" else "norm.") + p[2]] = v
        elif p[0].startswith("norm") and p[0][4:].isdigit():
            out[f"hidden_states_norms.stage{int(p[0][4:]) + 1}.{p[1]}"] = v
        elif p[0] == "layers" and p[2] == "downsample":
            out[f"swin.encoder.layers.{p[1]}.downsample." + ".".join(p[3:])] = v
        elif p[0] == "layers" and p[2] == "blocks":
            base = f"swin.encoder.layers.{p[1]}.blocks.{p[3]}."
            rest = ".".join(p[4:])
            if rest == "attn.relative_position_bias_table":
                out[base + "attention.relative_position_bias.relative_position_bias_table"] = v
            elif rest == "attn.relative_position_index":
                continue
            elif rest.startswith("attn.qkv."):
                C = v.shape[0] // 3
                for i, n in enumerate("qkv"):
                    out[base + f"attention.{n}_proj.{p[-1]}"] = v[i * C:(i + 1) * C]
            else:
                stem, leaf = rest.rsplit(".", 1)
                if stem not in leaf_map:
                    raise L.OmgHipError(f"swin_from_groundingdino: unknown key backbone.0.{k}")
                out[base + leaf_map[stem] + "." + leaf] = v
        else:
            raise L.OmgHipError(f"swin_from_groundingdino: unknown key backbone.0.{k}")
    return out


class SwinBackboneOutput:
    def __init__(self, feature_maps: Tuple[torch.Tensor, ...]):
        self.feature_maps = feature_maps
        self.hidden_states = None
        self.attentions = None


class SwinBackbone(FlatWeights):
    """``SwinBackbone(config, dtype, device)``; ``config``: the library's ``SwinConfig``, its dict, or a ``GroundingDinoConfig``.
    ``load_state_dict`` takes ``sd`` under the library's names or the Hub checkpoints' names; ``prefix="model.backbone.conv_encoder.model."``
    takes the backbone out of a ``GroundingDinoForObjectDetection`` state dict (its other keys are ignored)."""

    check_config = staticmethod(check_config)
    no_training = "dropout, 'drop_path_rate'"

    def __init__(self, config, dtype=torch.float16, device=None):
        super().__init__(config, dtype, device)
        self.out_features = list(self.cfg["out_features"])
        self.channels = [self.cfg["embed_dim"] << (int(s[5:]) - 1) for s in self.out_features]

    # ------------------------------------------------------------------ parameters
    def shapes(self) -> Dict[str, tuple]:
        c = self.cfg
        E, S = c["embed_dim"], c["window_size"]
        out = {"swin.embeddings.patch_embeddings.projection.weight": (E, 3, 4, 4), "swin.embeddings.patch_embeddings.projection.bias": (E,),
               "swin.embeddings.norm.weight": (E,), "swin.embeddings.norm.bias": (E,)}
        n = len(c["depths"])
        for li, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
            C = E << li
            M = int(c["mlp_ratio"] * C)
            for bi in range(depth):
                p = f"swin.encoder.layers.{li}.blocks.{bi}."
                for nm in ("q_proj", "k_proj", "v_proj", "o_proj"):
                    out[p + f"attention.{nm}.weight"], out[p + f"attention.{nm}.bias"] = (C, C), (C,)
                out[p + "attention.relative_position_bias.relative_position_bias_table"] = ((2 * S - 1) ** 2, heads)
                for nm in ("layernorm_before", "layernorm_after"):
                    out[p + nm + ".weight"], out[p + nm + ".bias"] = (C,), (C,)
                out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = (M, C), (M,)
                out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = (C, M), (C,)
            if li < n - 1:
                p = f"swin.encoder.layers.{li}.downsample."
                out[p + "reduction.weight"], out[p + "norm.weight"], out[p + "norm.bias"] = (2 * C, 4 * C), (4 * C,), (4 * C,)
        for st in c["out_features"]:
            C = E << (int(st[5:]) - 1)
            out[f"hidden_states_norms.{st}.weight"], out[f"hidden_states_norms.{st}.bias"] = (C,), (C,)
        return out

    @staticmethod
    def canonical_key(k: str, prefix: str = "") -> Optional[str]:
        """A checkpoint key -> this module's key; None for what is ignored (a stored relative_position_index, SwinModel's final
        layernorm, keys outside ``prefix``)."""
        k = FlatWeights.canonical_key(k, prefix)
        if k is None or k.endswith("relative_position_index") or k.startswith("swin.layernorm."):
            return None
        for a, b in _HUB_NAMES:
            if a in k:
                return k.replace(a, b)
        return k

    def _misshapen(self, k, ck):
        return k, " (interpolating a relative-position table is not built: 'window_size')" if ck.endswith("relative_position_bias_table") else ""

    # ------------------------------------------------------------------ kernel operands that are not the checkpoint's own tensors, built once
    def _pack(self) -> dict:
        w, E = self._w, self.cfg["embed_dim"]
        pk = {}
        pw = torch.zeros((E, PATCH_K), dtype=self._dtype, device=self._device)
        pw[:, :48] = w["swin.embeddings.patch_embeddings.projection.weight"].reshape(E, 48)
        pk["patch"] = pw
        for li, depth in enumerate(self.cfg["depths"]):
            for bi in range(depth):
                a = f"swin.encoder.layers.{li}.blocks.{bi}.attention."
                pk[a + "qkv.weight"] = torch.cat([w[a + f"{n}_proj.weight"] for n in "qkv"], dim=0).contiguous()
                pk[a + "qkv.bias"] = torch.cat([w[a + f"{n}_proj.bias"] for n in "qkv"], dim=0).contiguous()
                pk[a + "pad_kv"] = pk[a + "qkv.bias"][(E << li):]                      # k | v of a padded position: the bias slices
        return pk

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward_features(self, pixel_values: torch.Tensor) -> Dict[str, object]:
        """NCHW pixel values -> {"embeddings" [B, h w, E], "stage1" .. "stageN" [B, h w, C] (before downsampling), "grids" [(h, w)] per
        stage, "feature_maps": the NCHW tuple, one per out_feature, through its hidden_states_norms}."""
        x = pixel_values
        if not x.is_cuda:
            raise L.OmgHipError("SwinBackbone needs its input on the MI355X (cuda/hip device); there is no CPU fallback")
        dt, c, w = self._dtype, self.cfg, self._w
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] < 1 or x.shape[3] < 1:
            raise L.OmgHipError(f"SwinBackbone: input {tuple(x.shape)} is not [B, 3, H, W] ('num_channels')")
        if x.dtype not in (torch.float32, dt):
            raise L.OmgHipError(f"SwinBackbone: pixel values must be float32 or {dt}, not {x.dtype}")
        B = x.shape[0]
        H, W = (x.shape[2] + 3) // 4, (x.shape[3] + 3) // 4
        pk = self._pk()
        S, eps, scale = c["window_size"], c["layer_norm_eps"], HEAD_DIM ** -0.5
        P = "swin.embeddings."
        rows = ops.swin_patch_embed(x.contiguous(), dt, PATCH_K)
        t = ops.gemm(rows, pk["patch"], bias=w[P + "patch_embeddings.projection.bias"])
        t = ops.layernorm(t, w[P + "norm.weight"], w[P + "norm.bias"], 1e-5)
        feats: Dict[str, object] = {"embeddings": t.view(B, H * W, -1), "grids": []}
        maps: List[torch.Tensor] = []
        n = len(c["depths"])
        for li, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
            C = c["embed_dim"] << li
            for bi in range(depth):
                p = f"swin.encoder.layers.{li}.blocks.{bi}."
                a = p + "attention."
                y = ops.layernorm(t, w[p + "layernorm_before.weight"], w[p + "layernorm_before.bias"], eps)
                qkv = ops.gemm(y, pk[a + "qkv.weight"], bias=pk[a + "qkv.bias"])
                o = ops.attn_swin(qkv, B, H, W, heads, w[a + "relative_position_bias.relative_position_bias_table"], scale, window=S,
                                  shift=0 if bi % 2 == 0 else S // 2, pad_kv=pk[a + "pad_kv"])
                t = ops.gemm(o, w[a + "o_proj.weight"], bias=w[a + "o_proj.bias"], residual=t)
                y = ops.layernorm(t, w[p + "layernorm_after.weight"], w[p + "layernorm_after.bias"], eps)
                u = ops.gemm(y, w[p + "mlp.fc1.weight"], bias=w[p + "mlp.fc1.bias"])
                ops.gelu_erf(u, out=u)
                t = ops.gemm(u, w[p + "mlp.fc2.weight"], bias=w[p + "mlp.fc2.bias"], residual=t)
            st = f"stage{li + 1}"
            feats[st] = t.view(B, H * W, C)
            feats["grids"].append((H, W))
            if st in c["out_features"]:
                f = ops.layernorm(t, w[f"hidden_states_norms.{st}.weight"], w[f"hidden_states_norms.{st}.bias"], 1e-5)
                maps.append(f.view(B, H, W, C).permute(0, 3, 1, 2))
            if li < n - 1:
                p = f"swin.encoder.layers.{li}.downsample."
                m = ops.swin_merge_ln(t.view(B, H, W, C), w[p + "norm.weight"], w[p + "norm.bias"], 1e-5)
                t = ops.gemm(m, w[p + "reduction.weight"])
                H, W = (H + 1) // 2, (W + 1) // 2
        feats["feature_maps"] = tuple(maps)
        return feats

    def forward(self, pixel_values: torch.Tensor, **_ignored) -> SwinBackboneOutput:
        """-> an object with ``.feature_maps``: NCHW (permuted views of the NHWC results), one per ``out_features``."""
        return SwinBackboneOutput(self.forward_features(pixel_values)["feature_maps"])
