"""The derived-operand contract of omg_amd/_checkpoint.py::PackedCache, without a GPU: every module that keeps operands derived from its
weights drops them when a state dict is loaded, or the model is moved or cast, THROUGH A PARENT — ``nn.Module.load_state_dict`` on a parent
never calls a child's ``load_state_dict``, only its ``_load_from_state_dict``.  Each case wraps the narrowest model the suite builds on the
CPU in a plain ``nn.Module``, plants a mark in every cache and acts on the parent only."""
import ast
import glob
import os

import pytest
import torch
from torch import nn

from omg_amd import dpt as hip_dpt
from omg_amd import sam
from omg_amd import segment_anything as sa
from omg_amd._checkpoint import PackedCache
from omg_amd.attention import Attention
from omg_amd.controlnet import ControlNetModel
from omg_amd.modules import pointer_epoch
from omg_amd.resampler import Resampler
from omg_amd.text_encoder import ClipTextConfig, ClipTextEncoder
from omg_amd.unet import UNet2DConditionModel, UNetConfig
from omg_amd.vae import AutoencoderKLDecoder, VaeConfig
from tests import dpt_torch as dt
from tests.effvit_xl_torch import load_fixture_xl
from tests.test_effvit_xl import narrow_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every attribute of the package that holds something computed from the weights; a module that carries one must be a PackedCache
CACHES = ("_packed", "_qkv", "_kv", "_qkv_slots", "_kv_slots", "_kv_cache", "_mx8", "_ip_cache", "_cond_cache")
DPT_KEY = "dpt.embeddings.backbone.bit.embedder.convolution.weight"


class Parent(nn.Module):
    def __init__(self, child):
        super().__init__()
        self.child = child


def _dpt():
    return hip_dpt.DPTForDepthEstimation(dt.hf_config_dict(dt.small_cfg(96)), dtype=torch.float16, device="cpu")


MODELS = {
    "effvit_sam": lambda: narrow_sam(load_fixture_xl()[1]),
    "sam_vit_b": lambda: sa.build_sam_vit_b(device="cpu"),
    "dpt": _dpt,
    "clip": lambda: ClipTextEncoder(ClipTextConfig(vocab_size=96, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
                                                   projection_dim=64, eos_token_id=95), dtype=torch.float16, device="cpu"),
    "resampler": lambda: Resampler(dim=128, depth=2, dim_head=64, heads=2, num_queries=16, embedding_dim=64, output_dim=96, ff_mult=4,
                                   dtype=torch.float16, device="cpu"),
    "vae": lambda: AutoencoderKLDecoder(VaeConfig.tiny(), dtype=torch.float16, device="cpu"),
    "controlnet": lambda: ControlNetModel(UNetConfig.tiny(), dtype=torch.float16, device="cpu"),
    "unet": lambda: UNet2DConditionModel(UNetConfig.tiny(), dtype=torch.float16, device="cpu"),
}


def holders(root):
    return [m for m in root.modules() if any(a in m.__dict__ for a in CACHES)]


def mark(root):
    """Plant a mark in every cache under ``root``; -> the mark and the modules that hold one (derived, not listed)."""
    stale = {"stale": True}
    hs = holders(root)
    for m in hs:
        for a in CACHES:
            if a in m.__dict__:
                setattr(m, a, stale)
    return stale, hs


def survivors(root, stale):
    return [f"{type(m).__name__}.{a}" for m in root.modules() for a in CACHES if m.__dict__.get(a) is stale]


def zeroed(model):
    """``torch.empty`` parameters hold whatever the allocator left: give the state dict defined values."""
    with torch.no_grad():
        for p in model.parameters():
            p.zero_()
    return model


@pytest.mark.parametrize("name", list(MODELS))
def test_a_load_a_move_or_a_cast_through_a_parent_drops_every_cache(name):
    parent = Parent(zeroed(MODELS[name]()))
    sd = {k: v.clone() for k, v in parent.state_dict().items()}
    acts = {"load_state_dict": lambda: parent.load_state_dict(sd), "load_state_dict(assign=True)": lambda: parent.load_state_dict(sd, assign=True),
            "to(bfloat16)": lambda: parent.to(torch.bfloat16)}
    for what, act in acts.items():
        stale, hs = mark(parent)
        assert hs and all(isinstance(m, PackedCache) for m in hs), [type(m).__name__ for m in hs if not isinstance(m, PackedCache)]
        assert len(survivors(parent, stale)) >= len(hs)
        act()
        assert survivors(parent, stale) == [], what
        assert not any(m.__dict__[a] for m in hs for a in CACHES if a in m.__dict__), what         # falsy: not built


def test_every_model_was_reached():
    """The eight cases cover every PackedCache class of the package but the flat-weight models, which tests/test_checkpoint_base.py,
    test_swin.py, test_bert.py and test_gdino.py reload."""
    seen = set()
    for name in ("effvit_sam", "dpt", "clip", "resampler", "vae", "controlnet", "unet"):
        seen |= {type(m).__name__ for m in holders(MODELS[name]())}
    seen |= {type(m).__name__ for m in holders(sa.build_sam_vit_b(device="meta"))}
    assert seen >= {"LiteMLA", "EfficientViTSamImageEncoder", "SamPromptEncoder", "SamMaskDecoder", "SamImageEncoderViT", "DPTForDepthEstimation",
                    "ClipTextEncoder", "Resampler", "AutoencoderKLDecoder", "_MidAttention", "ControlNetConditioningEmbedding", "ControlNetModel",
                    "UNet2DConditionModel", "Attention", "Linear", "Conv2d", "GEGLU"}, seen


def test_dpt_refolds_from_the_state_dict_a_parent_loads():
    sd_a = {k: v.clone() for k, v in dt.seed_state(dt.DPTHybrid(dt.small_cfg(96)).eval(), 1).state_dict().items()}
    sd_b = {k: v.clone() for k, v in sd_a.items()}
    sd_b[DPT_KEY] = sd_a[DPT_KEY] + 0.05 * torch.randn(sd_a[DPT_KEY].shape, generator=torch.Generator().manual_seed(2))
    h = _dpt()
    parent = Parent(h)
    parent.load_state_dict({"child." + k: v for k, v in sd_a.items()})
    assert torch.equal(h._folded[DPT_KEY], dt.standardize(sd_a[DPT_KEY]))
    parent.load_state_dict({"child." + k: v for k, v in sd_b.items()})
    want = dt.standardize(sd_b[DPT_KEY])
    assert not torch.equal(want, dt.standardize(sd_a[DPT_KEY]))
    assert h._folded[DPT_KEY].dtype == torch.float32 and torch.equal(h._folded[DPT_KEY], want)       # from the checkpoint's own precision
    parent.to(torch.bfloat16)
    assert h._folded[DPT_KEY].dtype == torch.float32 and torch.equal(h._folded[DPT_KEY], want)       # survives .to()
    parent.load_state_dict({"child." + k: v for k, v in sd_b.items() if k != DPT_KEY}, strict=False)
    assert DPT_KEY not in h._folded and h._folded                                                    # absent for a key the state dict does not carry


@pytest.mark.parametrize("name", ["unet", "controlnet"])
def test_a_load_through_a_parent_counts_once_and_moves_the_pointer_epoch_with_what_was_packed(name):
    net = zeroed(MODELS[name]())
    parent = Parent(net)
    sd = parent.state_dict()

    def load():
        e, v = pointer_epoch(), getattr(net, "weights_version", 0)
        parent.load_state_dict(sd)
        assert net.weights_version == v + 1                         # exactly one per load
        return pointer_epoch() - e

    # Attention moves the epoch on every invalidation, packed or not (LoraBank.build and .to() rely on it): that is the idle figure.
    # Everything else moves it when, and only when, it had something packed: one step per packed holder.
    idle = load()
    assert load() == idle
    conv, other = net.conv_in, net.down_blocks[0].resnets[0].conv1
    conv._packed["w"] = torch.zeros(1)
    assert load() == idle + 1 and not conv._packed
    conv._packed["w"], other._packed["w"] = torch.zeros(1), torch.zeros(1)
    assert load() == idle + 2
    assert load() == idle
    # a subtree without Attention: not at all, then once
    sub = [m for m in net.modules() if not isinstance(m, Attention) and not any(isinstance(c, Attention) for c in m.modules()) and holders(m)][0]
    parent = Parent(sub)
    sd = parent.state_dict()
    e = pointer_epoch()
    parent.load_state_dict(sd)
    assert pointer_epoch() == e
    next(m for m in sub.modules() if hasattr(m, "packed_weight"))._packed["w"] = torch.zeros(1)
    parent.load_state_dict(sd)
    assert pointer_epoch() == e + 1


def _classes():
    for path in sorted(glob.glob(os.path.join(ROOT, "omg_amd", "*.py"))):
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.ClassDef):
                yield node.name, {f.name for f in node.body if isinstance(f, ast.FunctionDef)}


def test_the_invalidation_rule_is_written_in_the_base_alone():
    classes = list(_classes())
    assert len(classes) > 50
    assert [n for n, fs in classes if {"_load_from_state_dict", "_apply"} <= fs] == ["PackedCache"]
    assert sorted(n for n, fs in classes if "load_state_dict" in fs) == ["FlatWeights", "GroundingDinoDecoderHead", "IPAdapter"]
