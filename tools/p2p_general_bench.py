"""A/B of a word-swap prompt-to-prompt call: protocol mode (materialised probabilities, one request after another — it cannot batch)
against the fused general path (the edit folded into V; eager and captured graphs, all requests in lock-step).

A full-width stage-1 call of `--steps` steps at 1024² with the controller of "a man on the road" -> "a woman on the road",
cross_replace_steps {"default_": 0.6, "road": (0.2, 0.9)}, `--requests` requests, synthetic weights.  The arms run interleaved
(protocol / fused eager / fused graph, `--rounds` times) after one untimed pass of each; every figure is seconds per image pair
(request), timed with device events around the whole call.  No threshold: the log is the result.

    python tools/p2p_general_bench.py [--tiny] [--steps 10] [--requests 8] [--rounds 2] > profiles/r09_p2p_general_ab.log
"""
import argparse
import contextlib
import io
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omg_amd import controller as pc                                                      # noqa: E402
from omg_amd.attention import RegionControlNet_AttnProcessor                              # noqa: E402
from omg_amd.pipeline import LoraMultiConceptPipeline, revise_regionally_controlnet_forward  # noqa: E402
from omg_amd.schedulers import make_scheduler                                             # noqa: E402
from omg_amd.synthetic import c2_inputs, c2_masks, make_concept_models                              # noqa: E402
from omg_amd.unet import UNet2DConditionModel, UNetConfig                                 # noqa: E402


class WordPieces:
    """A whitespace tokenizer with the two methods the aligner uses (encode with BOS / EOS, decode of one id)."""

    def __init__(self):
        self.words = ["<s>", "</s>"]

    def encode(self, text):
        ids = []
        for w in text.split(" "):
            if w not in self.words:
                self.words.append(w)
            ids.append(self.words.index(w))
        return [0] + ids + [1]

    def decode(self, ids):
        return " ".join(self.words[i] for i in ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--requests", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    dev, dt = torch.device("cuda", 0), torch.float16
    cfg = UNetConfig.tiny() if args.tiny else UNetConfig.sdxl()
    unet = UNet2DConditionModel(cfg, dtype=dt, device=dev).init_synthetic_(seed=0)
    HW = cfg.sample_size * 8
    ctl = pc.AttentionReplace(["a man on the road", "a woman on the road"], args.steps, {"default_": 0.6, "road": (0.2, 0.9)}, 0.4,
                              width=HW // 32, height=HW // 32, tokenizer=WordPieces(), device=dev, dtype=dt)
    with contextlib.redirect_stdout(io.StringIO()):
        revise_regionally_controlnet_forward(unet, ctl)
    assert not ctl.is_pure_replacement
    concept = make_concept_models(unet, n_concepts=2, rank=8 if args.tiny else 64)
    pipe = LoraMultiConceptPipeline(unet, make_scheduler("ddim"))
    reqs = [c2_inputs(unet, seed=j, height=HW, width=HW) for j in range(args.requests)]
    masks = c2_masks(HW, HW, device=dev)
    for r in reqs:
        r["region_masks"] = masks
    common = dict(height=HW, width=HW, num_inference_steps=args.steps, guidance_scale=7.5, cross_attention_kwargs={"scale": 0.8},
                  controller=ctl, concept_models=concept, stage=1, lora_list=["concept0", "concept1"], styleL=False)

    def call(batches, use_graph):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for b in batches:
            ctl.reset()
            pipe.generate_many(b, use_graph=use_graph, **common)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / 1e3 / args.requests

    arms = {"protocol, one request at a time": (True, [[r] for r in reqs], False),
            "fused, eager, lock-step": (False, [reqs], False),
            "fused, graph, lock-step": (False, [reqs], True)}
    print(f"# word-swap stage-1 call: {args.steps} steps, {HW}x{HW}, {args.requests} requests, fp16, {torch.cuda.get_device_name(0)}")
    print("# seconds per request (image pair); pass 0 is the untimed warm-up of every arm (lazy inits, graph capture)")
    for rnd in range(args.rounds + 1):
        for name, (protocol, batches, use_graph) in arms.items():
            RegionControlNet_AttnProcessor.force_protocol = protocol
            try:
                s = call(batches, use_graph)
            finally:
                RegionControlNet_AttnProcessor.force_protocol = False
            print(f"pass {rnd}{' (warm-up)' if rnd == 0 else ''}: {name:34s} {s:9.4f} s/request", flush=True)


if __name__ == "__main__":
    main()
