#!/usr/bin/env python
"""End-to-end cost of conv LoRA: one stage-2 call at the benchmark configuration (SDXL 1024^2, 50 DDIM steps, 8 requests in lock-step, 2 concepts
with masked fusion, merged mode, hipGraph replay, no VAE) with synthetic adapters ``make_synthetic_adapter(conv=True)`` against ``conv=False``.
The two banks live on one UNet in turn (conv=False, conv=True, conv=False, conv=True); every turn rebuilds its slot stacks, runs one untimed call
(graph capture) and ``--calls`` timed ones.  Reports seconds per denoising step and the HBM the conv stacks add.

    python tools/conv_lora_e2e.py [--calls 1] [--out profiles/conv_lora_e2e.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omg_amd import controller as pc                                                         # noqa: E402
from omg_amd.lora import LoraBank, make_synthetic_adapter                                     # noqa: E402
from omg_amd.modules import Conv2d                                                            # noqa: E402
from omg_amd.pipeline import ConceptModels, LoraMultiConceptPipeline, revise_regionally_controlnet_forward   # noqa: E402
from omg_amd.schedulers import make_scheduler                                                 # noqa: E402
from omg_amd.synthetic import c2_inputs, c2_masks                                             # noqa: E402
from omg_amd.unet import UNet2DConditionModel, UNetConfig                                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1, help="timed stage-2 calls per turn")
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--images-per-step", type=int, default=8)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--tiny", action="store_true", help="debug: tiny UNet")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev, dt = torch.device("cuda:0"), torch.float16
    cfg = UNetConfig.tiny() if a.tiny else UNetConfig.sdxl()
    unet = UNet2DConditionModel(cfg, dtype=dt, device=dev).init_synthetic_(seed=0)
    HW = cfg.sample_size * 8
    P = "a man and a woman walking on the street"
    ctl = pc.AttentionReplace([P, P], a.denoise_steps, cross_replace_steps={"default_": 1.0}, self_replace_steps=0.4, width=HW // 32, height=HW // 32,
                              device=dev, dtype=dt)
    with contextlib.redirect_stdout(io.StringIO()):
        revise_regionally_controlnet_forward(unet, ctl)
    pipe = LoraMultiConceptPipeline(unet, make_scheduler("ddim"))
    masks = c2_masks(HW, HW, device=dev)
    rank = a.rank if not a.tiny else 8

    def requests(i):
        reqs = []
        for j in range(a.images_per_step):
            r = c2_inputs(unet, seed=i * 16 + j, height=HW, width=HW)
            r["region_masks"] = masks
            reqs.append(r)
        return reqs

    def call(concept, reqs):
        ctl.reset()
        return pipe.generate_many(reqs, height=HW, width=HW, num_inference_steps=a.denoise_steps, guidance_scale=7.5, cross_attention_kwargs={"scale": 0.8},
                                  controller=ctl, concept_models=concept, stage=2, lora_list=["concept0", "concept1"], styleL=False, use_graph=True)

    turns = []
    for turn, conv in enumerate((False, True, False, True)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        m0 = torch.cuda.memory_allocated()
        adapters = [make_synthetic_adapter(unet, f"concept{c}", rank, seed=1000 + c, conv=conv) for c in range(2)]
        bank = LoraBank(unet, adapters)
        concept = ConceptModels(unet, bank)
        lat = call(concept, requests(0))                                     # builds the slot stacks, captures the step graphs
        torch.cuda.synchronize()
        m1 = torch.cuda.memory_allocated()
        stacks = sum(t.numel() * t.element_size() for m in unet.modules() if isinstance(m, Conv2d)
                     for t in (m.w_slots, m.lora_down, m.lora_up) if t is not None)
        t0 = time.perf_counter()
        for i in range(a.calls):
            lat = call(concept, requests(1 + i))
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / a.calls
        assert torch.isfinite(lat).all()
        row = dict(turn=turn, conv=conv, s_per_call=round(el, 4), s_per_step=round(el / a.denoise_steps, 5), images_per_s=round(a.images_per_step / el, 4),
                   conv_stack_bytes=stacks, allocated_after_first_call_gb=round((m1 - m0) / 1e9, 3),
                   conv_targets=sum(1 for k in adapters[0].weights if adapters[0].weights[k][0].dim() == 4), checksum=float(lat.float().abs().mean()))
        turns.append(row)
        print(json.dumps(row), flush=True)
        bank.clear()
        del bank, concept, adapters, lat
    f = [t["s_per_step"] for t in turns if not t["conv"]]
    c = [t["s_per_step"] for t in turns if t["conv"]]
    summary = dict(what="one stage-2 call, benchmark configuration, merged mode, no VAE", rank=rank, images_per_step=a.images_per_step, denoise_steps=a.denoise_steps,
                   s_per_step_conv_false=f, s_per_step_conv_true=c, ratio=round((sum(c) / len(c)) / (sum(f) / len(f)), 4),
                   added_hbm_gb=round(turns[1]["conv_stack_bytes"] / 1e9, 3), turns=turns)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
