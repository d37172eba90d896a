"""Checkpoint plumbing the models share: the reader of a local checkpoint directory, the parameter holders of the models that keep the
checkpoint's module tree (``param``, ``Weight``, ``Seq``), :class:`PackedCache`, the base of every module that keeps operands derived
from its weights, and :class:`FlatWeights`, the base of the models that keep their parameters in one flat dict under the checkpoint's
key names (``SwinBackbone``, ``BertTextEncoder``, ``GroundingDinoEncoder``, ``GroundingDinoDecoderHead``).  No kernel is called from here.

The derived-operand contract.  Fused q|k|v stacks, BatchNorm-folded and repacked convolution weights, the dense positional encoding and
their like are computed once from the weights and reused by every forward; their holder is a :class:`PackedCache` and drops them in
``invalidate_packed()``.  The base calls that from ``_load_from_state_dict`` and ``_apply`` — the two hooks torch runs on EVERY
descendant, whichever module ``load_state_dict``, ``.to()`` or ``.half()`` was called on — and nowhere else in the package is the rule
written: no holder overrides ``load_state_dict`` for it, and nobody assigns another module's cache.  No hook sees an in-place write to
a parameter (``p.data.copy_(...)``): whoever writes one calls ``invalidate_packed()`` afterwards, as the ``init_synthetic_`` methods do.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib as L

__all__ = ["read_checkpoint", "param", "Weight", "Seq", "PackedCache", "FlatWeights"]


def read_checkpoint(path, who):
    """A local checkpoint directory -> (the dict of its ``config.json``, the state dict of its ``model.safetensors`` or
    ``pytorch_model.bin`` on the CPU).  ``who`` is the class the error names."""
    path = os.fspath(path)
    cfg_file = os.path.join(path, "config.json")
    if not os.path.isdir(path) or not os.path.exists(cfg_file):
        raise L.OmgHipError(f"{who}.from_pretrained: {path} is not a local checkpoint directory with a config.json (nothing is downloaded)")
    with open(cfg_file) as f:
        config = json.load(f)
    st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd = load_file(st, device="cpu")
    elif os.path.exists(pt):
        sd = torch.load(pt, map_location="cpu", weights_only=True)
    else:
        raise L.OmgHipError(f"{who}.from_pretrained: neither model.safetensors nor pytorch_model.bin in {path}")
    return config, sd


# ------------------------------------------------------------------------------------------------ holders of a checkpoint's module tree
def param(shape, dtype, device):
    return nn.Parameter(torch.zeros(shape, dtype=dtype, device=device), requires_grad=False)


class Weight(nn.Module):
    """Holder of ``weight`` (+ ``bias``): an Embedding, Linear, LayerNorm or convolution of the checkpoint."""

    def __init__(self, shape, bias, dtype, device):
        super().__init__()
        self.weight = param(shape, dtype, device)
        if bias:
            self.bias = param((bias,), dtype, device)


class Seq(nn.Module):
    """Children under the indices of an nn.Sequential: a list, or ``{index: module}`` where the activations in between hold no weights."""

    def __init__(self, mods):
        super().__init__()
        for i, m in (mods.items() if isinstance(mods, dict) else enumerate(mods)):
            self.add_module(str(i), m)

    def __getitem__(self, i):
        return getattr(self, str(i))


# ------------------------------------------------------------------------------------------------ operands derived from the weights
class PackedCache(nn.Module):
    """A module that keeps ``self._packed``: kernel operands derived from its weights, built once by ``_pk()`` from ``_pack()`` and
    dropped by ``invalidate_packed()`` whenever a state dict is loaded or the module is moved or cast, through whichever ancestor.
    Falsy (None, {}) means not built.  A holder that builds everything at once returns the whole dict from ``_pack()``; one that
    fills per key keeps the default and fills the dict ``_pk()`` hands it.  A subclass that derives more than ``_packed`` from its
    weights extends ``invalidate_packed()``."""

    def __init__(self):
        super().__init__()
        self._packed: Optional[dict] = None

    def _pack(self) -> dict:
        return {}

    def _pk(self) -> dict:
        if not self._packed:
            self._packed = self._pack()
        return self._packed

    def invalidate_packed(self) -> None:
        self._packed = None

    def _load_from_state_dict(self, *a, **k):
        self.invalidate_packed()
        return super()._load_from_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self.invalidate_packed()
        return super()._apply(fn, *a, **k)


# ------------------------------------------------------------------------------------------------ parameters in one flat dict
class FlatWeights(PackedCache):
    """An inference-only module whose parameters are ``self._w``: one dict of tensors under the checkpoint's own key names, in the order
    and with the shapes of ``shapes()``.  A model supplies ``check_config`` (a static method: the checkpoint's config -> the dict kept as
    ``self.cfg``), ``shapes()``, ``_pack()`` (the kernel operands that are not the checkpoint's own tensors; ``_pk()`` builds them once
    and every reload or move drops them) and ``forward``, and sets ``prefix`` and ``no_training``.  What a loader does differently goes
    into ``canonical_key``, ``_unexpected`` and ``_misshapen``."""

    prefix = ""                          # from_pretrained's default: where the module's keys start in its usual checkpoint
    no_training = "dropout"              # what of training is not built, for train(True)'s refusal
    constructor_keywords: Tuple[str, ...] = ()      # keywords from_pretrained hands to the constructor; it ignores all others

    def __init__(self, config, dtype=torch.float16, device=None):
        super().__init__()
        if dtype not in (torch.float16, torch.bfloat16):
            raise L.OmgHipError(f"{type(self).__name__}: dtype {dtype}; the kernels store float16 or bfloat16")
        self.cfg = self.check_config(config)
        self._dtype, self._device = dtype, torch.device(device) if device is not None else torch.device("cpu")
        self._w: Dict[str, torch.Tensor] = {k: torch.zeros(s, dtype=dtype, device=self._device) for k, s in self.shapes().items()}
        self.eval()

    def shapes(self) -> Dict[str, tuple]:
        raise NotImplementedError

    def _pack(self) -> dict:
        raise NotImplementedError

    def state_dict(self, *a, **k):
        return dict(self._w)

    # ------------------------------------------------------------------ loading
    @staticmethod
    def canonical_key(k: str, prefix: str = "") -> Optional[str]:
        """A checkpoint key -> this module's key; None for what is ignored (keys outside ``prefix``)."""
        return k[len(prefix):] if k.startswith(prefix) else None

    def _unexpected(self, k: str, ck: str) -> Optional[str]:
        """The name under which the checkpoint key ``k`` (``ck`` under ``prefix``, not one of ``shapes()``) is reported as unexpected;
        None where it is another module's."""
        return k

    def _misshapen(self, k: str, ck: str) -> Tuple[str, str]:
        """(the name a shape error gives the checkpoint key ``k`` of this module's ``ck``, a hint behind the message)."""
        return ck, ""

    def load_state_dict(self, sd, strict: bool = True, prefix: str = ""):
        """``sd`` under the checkpoint's names; ``prefix`` takes this module's keys out of a larger model's state dict and ignores the
        others.  -> (missing, unexpected); with ``strict`` either raises."""
        who = type(self).__name__
        shapes = self.shapes()
        seen, unexpected = set(), []
        for k, v in sd.items():
            ck = self.canonical_key(k, prefix)
            if ck is None:
                continue
            if ck not in shapes:
                name = self._unexpected(k, ck)
                if name is not None:
                    unexpected.append(name)
                continue
            if tuple(v.shape) != tuple(shapes[ck]):
                name, hint = self._misshapen(k, ck)
                raise L.OmgHipError(f"{who}.load_state_dict: {name} is {tuple(v.shape)}, the config needs {tuple(shapes[ck])}{hint}")
            self._w[ck] = v.detach().to(device=self._device, dtype=self._dtype).contiguous().clone()
            seen.add(ck)
        missing: List[str] = [k for k in shapes if k not in seen]
        if strict and (missing or unexpected):
            raise L.OmgHipError(f"{who}.load_state_dict: missing {missing[:6]}{' ...' if len(missing) > 6 else ''}, "
                                f"unexpected {unexpected[:6]}{' ...' if len(unexpected) > 6 else ''}")
        self.invalidate_packed()
        return missing, unexpected

    @classmethod
    def from_state_dict(cls, config, sd, torch_dtype=torch.float16, device=None, prefix: Optional[str] = None, **keywords):
        """What ``from_pretrained`` builds, from a checkpoint that is already read: its config and its state dict."""
        model = cls(config, dtype=torch_dtype, device=device, **{k: v for k, v in keywords.items() if k in cls.constructor_keywords})
        model.load_state_dict(sd, strict=True, prefix=cls.prefix if prefix is None else prefix)
        return model

    @classmethod
    def from_pretrained(cls, path, torch_dtype=torch.float16, device=None, prefix: Optional[str] = None, **keywords):
        """A local checkpoint directory: ``config.json`` and ``model.safetensors`` or ``pytorch_model.bin``.  ``prefix``: the class's own
        unless given.  Keywords the constructor does not take (the library's ``from_pretrained`` takes many) are ignored."""
        config, sd = read_checkpoint(path, cls.__name__)
        return cls.from_state_dict(config, sd, torch_dtype=torch_dtype, device=device, prefix=prefix, **keywords)

    # ------------------------------------------------------------------ nn.Module
    def train(self, mode: bool = True):
        if mode:
            raise L.OmgHipError(f"{type(self).__name__}: training ({self.no_training}) is not built; the module is inference only")
        return super().train(False)

    def _apply(self, fn, *a, **k):
        self._w = {key: fn(t) for key, t in self._w.items()}
        any_t = next(iter(self._w.values()))
        self._dtype, self._device = any_t.dtype, any_t.device
        return super()._apply(fn, *a, **k)

    @property
    def dtype(self):
        return self._dtype
