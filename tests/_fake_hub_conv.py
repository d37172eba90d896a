"""LoRA files with convolution entries for the fake hub of tests/_fake_hub.py: the file `write_lora_file` writes, plus a LoCon pair for every
conv target of the UNet — kohya style with SGM block names (``in_layers_2``, ``out_layers_3``, ``skip_connection``, ``op``, ``conv``) and a
per-layer alpha, or PEFT style; the up weights are stored as 1x1 convolutions, as such files hold them."""
import re

import torch
from safetensors.torch import load_file, save_file

from tests import _fake_hub as hub

_RES = {"conv1": "in_layers_2", "conv2": "out_layers_3", "conv_shortcut": "skip_connection"}


def sgm_flat_conv(unet, mod: str) -> str:
    """``down_blocks.1.resnets.0.conv_shortcut`` -> ``input_blocks_4_0_skip_connection`` (the SGM name of a conv module)."""
    m = re.match(r"^down_blocks\.(\d+)\.downsamplers\.0\.conv$", mod)
    if m:
        return f"input_blocks_{3 * (int(m[1]) + 1)}_0_op"
    m = re.match(r"^up_blocks\.(\d+)\.upsamplers\.0\.conv$", mod)
    if m:
        b = int(m[1])
        return f"output_blocks_{3 * b + 2}_{2 if unet.up_blocks[b].has_attn else 1}_conv"
    head, leaf = mod.rsplit(".", 1)
    return hub.sgm_flat(head + ".X")[:-1] + _RES[leaf]


def write_conv_lora_file(path, unet, seed, rank=4, style="kohya", text_encoders=None, conv_scale=0.1):
    """`hub.write_lora_file(...)` + conv entries.  Returns ``(path, conv)`` with ``conv[module] = (A [r, Cin, k, k], B [Cout, r])`` as written
    (alpha = rank, so the loader's fold is the identity)."""
    from omg_amd.loaders import conv_module_paths
    hub.write_lora_file(path, unet, seed, rank=rank, style=style, text_encoders=text_encoders)
    sd = load_file(path)
    g = torch.Generator().manual_seed(seed + 5000)
    conv = {}
    for mod, (cin, cout, k) in conv_module_paths(unet).items():
        a = torch.randn(rank, cin, k, k, generator=g) * (cin * k * k) ** -0.5
        b = torch.randn(cout, rank, generator=g) * conv_scale
        conv[mod] = (a, b)
        if style == "kohya":
            f = "lora_unet_" + sgm_flat_conv(unet, mod)
            sd[f + ".lora_down.weight"], sd[f + ".lora_up.weight"], sd[f + ".alpha"] = a, b[:, :, None, None], torch.tensor(float(rank))
        else:
            sd[f"unet.{mod}.lora_A.weight"], sd[f"unet.{mod}.lora_B.weight"] = a, b[:, :, None, None]
    save_file({k: v.contiguous() for k, v in sd.items()}, path)
    return path, conv
